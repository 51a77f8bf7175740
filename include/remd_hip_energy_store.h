/*
 * remd_hip_energy_store.h — GPU-only extension of the C ABI in remd_hip.h: the stored energies and state indices of a multistate run
 * on the device, and the three passes of multistate/analysis.py that walk them.
 *
 * A store holds the reporter's own records, uploaded once and in the reporter's own layouts (no transposition on the host):
 *
 *   energies  [T][R][S]   reduced potential of replica r at iteration t, evaluated in the sampled state s
 *   unsampled [T][R][U]   the same in the U unsampled end states; U is 0 or 2
 *   states    [T][R]      the state replica r occupies at iteration t, 0 ... S - 1
 *
 * Effective energy (MultiStateSamplerAnalyzer.get_effective_energy_timeseries).  With s(t, r) = states[t][r]:
 *
 *   u_n[t] = e(t) + ( -w(t) + L(t) )                     (without the weights: u_n[t] = e(t))
 *   e(t)   = sum_r energies[t][r][s(t, r)]               plain ascending r, starting from 0.0
 *   w(t)   = sum_r log_weights[t][s(t, r)]               plain ascending r, starting from 0.0
 *   L(t)   = log( sum_s exp(a_s - m) ) + m               a_s = -f_l[s] + log_weights[t][s]; plain ascending s, starting from 0.0;
 *                                                        m = max_s a_s where that is finite, else 0 (analysis._logsumexp)
 *
 * Everything is f64; the order above is the whole definition, so e(t) and w(t) are reproducible to the bit by any host that adds
 * in ascending r.  L(t) differs from a host's only by the rounding of exp and log.  Non-finite terms propagate as IEEE arithmetic
 * does: an occupied +inf gives +inf, +inf next to -inf gives NaN, a NaN gives NaN.
 *
 * u_ln gather (MultiStateSamplerAnalyzer._compute_mbar_decorrelated_energies).  For a selection iterations[n_sel] the matrix MBAR
 * takes, [U + S][R * n_sel]: column r * n_sel + j is (iteration iterations[j], replica r); for U == 2 row 0 is unsampled[..][0],
 * rows 1 ... S the sampled states, row S + 1 unsampled[..][1]; for U == 0 the S rows alone.  Values are copied as 64-bit words:
 * infinities and NaN payloads come through unchanged.  N_l[first + s] (first = U / 2) counts the selected (iteration, replica) pairs
 * in state s; the end rows get 0.
 *
 * Transition counts (generate_mixing_statistics).  n_ij[a][b] = the number of (t, r) with t_begin <= t < t_end - 1,
 * states[t][r] == a and states[t + 1][r] == b.  Integer counters only: exact, whatever the order.
 *
 * Statistical inefficiency of several series (analysis.statistical_inefficiency_multiple for K series of one length N).  With the
 * pooled mean mu = sum_kn A / (K N), sigma2 = sum_kn (A - mu)^2 / (K N) and dA = A - mu:
 *
 *   C(t) = sum_k sum_{n = 0}^{N - t - 1} dA_kn dA_k,n+t / (K (N - t) sigma2)
 *   g    = 1 + sum_t 2 C(t) (1 - t / N) increment(t)     over the lags t = 1, 2, 3, ... (increment 1), or with `fast`
 *                                                        t = 1, 2, 4, 7, 11, ... (the increment grows by 1 per lag)
 *
 * summed until the first C(t) <= 0 at a lag t > mintime, or until t >= N - 1; the result is max(g, 1).  As in
 * remd_hip_timeseries.h no pass uses a floating-point atomic: every sum is taken per (series, chunk of samples), the chunks are cut
 * at absolute sample indices and merged in the order (series, chunk), so g depends on the data alone: not on how the lags were
 * batched, and it is identical from run to run.
 *
 * A store is an object of its own: it needs a device, not a remd_handle.  A failed call returns non-zero and leaves its message in
 * remd_last_error(NULL); the store stays usable.
 *
 * These entry points are declared here and not in remd_hip.h because the CPU port of the ABI does not provide them: a host binds
 * them only where the loaded library exports them.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_ENERGY_STORE_H
#define REMD_HIP_ENERGY_STORE_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most lags of one batch of remd_series_inefficiency_multiple: batches of 8, 16, 32, then 64 lags until the walk stops */
#define REMD_SERIES_MAX_BATCH 64

typedef struct remd_energy_store_ctx* remd_energy_store;

/* Uploads the three arrays once.  Refused: T < 1, R < 1, S < 1, U other than 0 or 2, a state index outside 0 ... S - 1.  Energies
   are not checked: +-inf and NaN are legal stored values.  unsampled may be NULL when U == 0.                                      */
int  remd_energy_store_create(int device, int64_t T, int32_t R, int32_t S, int32_t U, const double* energies, const double* unsampled,
                              const int32_t* states, remd_energy_store* out);
void remd_energy_store_destroy(remd_energy_store store);

/* u_n[T] as defined above.  log_weights [T][S] and f_l [S]: both, or both NULL; one alone is refused.                              */
int  remd_energy_store_effective_energy(remd_energy_store store, const double* log_weights, const double* f_l, double* u_n);

/* u_ln [U + S][R * n_sel] and N_l [U + S] of the selection iterations[n_sel] (any order, repeats allowed).  Refused: n_sel < 0, an
   iteration outside 0 ... T - 1.  n_sel == 0 is legal: it writes nothing to u_ln and zeros to N_l.                                 */
int  remd_energy_store_gather_u_ln(remd_energy_store store, int64_t n_sel, const int64_t* iterations, double* u_ln, int64_t* N_l);

/* n_ij [S][S] over the iterations [t_begin, t_end).  Refused: a range outside 0 ... T (t_begin < 0, t_end > T, t_begin > t_end).
   A range with fewer than two iterations returns zeros.                                                                            */
int  remd_energy_store_transition_counts(remd_energy_store store, int64_t t_begin, int64_t t_end, int64_t* n_ij);

/* The work split of every pass, for tests and tools:
     effective_chunk   iterations per workgroup of the effective-energy pass (one thread per iteration)
     gather_tile       the gather moves tiles of gather_tile selected iterations x gather_tile states through the LDS
     count_chunk       (iteration, replica) pairs per workgroup of the counting passes (transition counts, N_l)
     hist_max_states   the counting passes keep a per-workgroup LDS histogram for S <= hist_max_states and add straight to the
                       result above it                                                                                              */
int  remd_energy_store_chunks(remd_energy_store store, int64_t* effective_chunk, int64_t* gather_tile, int64_t* count_chunk,
                              int32_t* hist_max_states);
/* device milliseconds of the kernels of the last pass on this store (events around the launches; transfers are not in it)          */
int  remd_energy_store_last_ms(remd_energy_store store, double* ms);

/* g of the K series A_kn [K][N]; fast != 0: the growing increments.  status: 0, or 1 for sigma2 == 0, where g is NaN (the host
   function raises there).  last_lag (or NULL): the last lag whose term was added to g, 0 if none was.
   Refused: K < 1, K > 65535 (a grid dimension), N < 2, a non-finite sample, mintime < 0.                                           */
int  remd_series_inefficiency_multiple(int device, int32_t K, int64_t N, const double* A_kn, int fast, int mintime, double* g,
                                       int32_t* status, int64_t* last_lag);
/* The same with the lags of the first batch chosen (1 ... REMD_SERIES_MAX_BATCH; it doubles per batch up to the maximum), and the
   device milliseconds of the kernels in ms (or NULL), for tests and tools: g does not depend on first_batch.
   chunk (or NULL): the samples per workgroup of every pass.                                                                        */
int  remd_series_inefficiency_multiple_batched(int device, int32_t K, int64_t N, const double* A_kn, int fast, int mintime,
                                               int32_t first_batch, double* g, int32_t* status, int64_t* last_lag, double* ms,
                                               int64_t* chunk);

#ifdef __cplusplus
}
#endif

#endif
