/*
 * remd_hip_mbar.h — GPU-only extension of the C ABI in remd_hip.h: the passes of the MBAR estimator on the device.
 *
 * The multistate Bennett acceptance ratio estimator (Shirts & Chodera 2008) as multistate/analysis.py::MBAR solves it, with the
 * passes over the [K][N] matrix of reduced potentials done on the device: the log of the mixture denominator per sample
 *
 *   log_den_n = ln sum_k N_k exp(f_k - u_kn)                  (over the sampled states, N_k > 0)
 *
 * the self-consistent update  f_i = -ln sum_n exp(-u_in - log_den_n)  (eq. 11), the sums the Newton step needs, the Gram matrix
 * W^T W of the weights  W_nk = exp(f_k - u_kn - log_den_n)  that the asymptotic covariance (eq. 8) needs, and the weights
 * themselves.  The K x K linear algebra stays with the host.  Everything is f64.  No pass uses a floating-point atomic: every
 * sum is taken per chunk of samples and the chunks are merged in chunk order, so a result depends on the input alone.
 *
 * An MBAR problem is an object of its own: it needs a device, not a remd_handle.  A failed call returns non-zero and leaves its
 * message in remd_last_error(NULL).
 *
 * These entry points are declared here and not in remd_hip.h because the CPU port of the ABI does not provide them: a host binds
 * them only where the loaded library exports them.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_MBAR_H
#define REMD_HIP_MBAR_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most states of one problem: the augmented Gram matrix of remd_mbar_gram then has 2 x 512 = 1024 columns */
#define REMD_MBAR_MAX_STATES 512

typedef struct remd_mbar_ctx* remd_mbar;

/* Uploads u_kn[K][N] (sample index fastest) and N_k[K] once.  Refused: K < 1 or N < 1, K > REMD_MBAR_MAX_STATES, a negative N_k,
   sum N_k != N, a non-finite u_kn in a row with N_k > 0.                                                                          */
int  remd_mbar_create(int device, int K, int64_t N, const double* u_kn, const int64_t* N_k, remd_mbar* out);
void remd_mbar_destroy(remd_mbar m);

/* log_den[N] (or NULL) at f_k[K], and the objective  phi = sum_n log_den_n - sum_k N_k f_k  (or NULL)                            */
int  remd_mbar_log_denominator(remd_mbar m, const double* f_k, double* log_den, double* phi);
/* one application of eq. 11 to every state, sampled or not, with the denominator at f_k:  f_new[K], not shifted                  */
int  remd_mbar_self_consistent(remd_mbar m, const double* f_k, double* f_new);
/* W_sum[K] = sum_n W_kn and gram[K][K] = W W^T at f_k; rows and columns of unsampled states are 0.  phi (or NULL) as above.      */
int  remd_mbar_newton_parts(remd_mbar m, const double* f_k, double* W_sum, double* gram, double* phi);
/* gram[C][C] = W^T W over all K states (C = K), or with_observable != 0: C = 2K, column K + k = exp(ln W_nk + ln A_kn - log_cA_k)
   with the observable A = u - (min u - 1) and log_cA_k = ln sum_n W_nk A_kn, returned in log_cA[K] (or NULL).                     */
int  remd_mbar_gram(remd_mbar m, const double* f_k, int with_observable, double* gram, double* log_cA);
/* The Gram matrix over the K stored states, L perturbed states and I observables of this call: what perturbed free energies and
   expectations with their uncertainties need (C = K + L + I columns, each a normalised weight of the N stored samples):
     columns 0 .. K-1        W_nk = exp(f_k - u_kn - log_den_n), as in remd_mbar_gram
     columns K .. K+L-1      exp(f_l - u_ln - log_den_n)  with  f_l = -ln sum_n exp(-u_ln - log_den_n)  (eq. 11), returned in f_l[L];
                             a +inf in u_ln gives that sample the weight 0 in that state
     columns K+L .. C-1      exp(ln W_n,s + ln A_in - log_cA_i)  with s = obs_state[i] a column below K + L and
                             log_cA_i = ln sum_n W_ns A_in, returned in log_cA[I]; A_in is the observable already shifted above 0
   u_ln[L][N] and A_in[I][N] (sample index fastest) are uploaded for the call and freed after it.  L or I may be 0 (its arrays NULL),
   not both.  Refused: a negative count, C > 2 x REMD_MBAR_MAX_STATES, a NaN or -inf in u_ln, a perturbed state whose weights all
   vanish, an obs_state outside 0 .. K+L-1, a non-positive or non-finite A_in.  The samples per workgroup are those
   remd_mbar_chunks reports: the row chunk for f_l and log_cA, the Gram chunk of C columns for the matrix.                        */
int  remd_mbar_augmented_gram(remd_mbar m, const double* f_k,
                              int L, const double* u_ln,
                              int I, const double* A_in, const int32_t* obs_state,
                              double* f_l, double* log_cA, double* gram);
/* log_W_nk[N][K] = f_k - u_kn - log_den_n, state index fastest                                                                   */
int  remd_mbar_log_weights(remd_mbar m, const double* f_k, double* log_W_nk);
/* the samples per workgroup of the column pass, the row pass and the Gram pass (C columns) of this problem, for tests and tools  */
int  remd_mbar_chunks(remd_mbar m, int C, int64_t* column_chunk, int64_t* row_chunk, int64_t* gram_chunk);
/* device milliseconds of the kernels of the last call on this object (events around its launches), for tools                     */
int  remd_mbar_last_ms(remd_mbar m, double* ms);

/* ---- bootstrap replicates -------------------------------------------------------------------------------------------------------
 * A bootstrap replicate of the problem resamples every sampled state's samples with replacement, N_k draws from the N_k samples of
 * state k.  It is kept as a vector of multiplicities c_n >= 0 over the N stored samples (sum of c_n over the samples of state k =
 * N_k), never as a gathered matrix, and enters every equation as the weight of sample n:
 *
 *   log_den_n  unchanged                                        f_i = -ln sum_n c_n exp(-u_in - log_den_n)
 *   W_sum_k = sum_n c_n W_kn                                    gram = W diag(c) W^T
 *   phi = sum_n c_n log_den_n - sum_k N_k f_k
 *
 * Draw j = 0 .. N_k - 1 of state k (its row of u_kn) in replicate t takes the Philox4x32-10 block of csrc/rng.h with the key `seed`
 * and the counter (a, b, t) = (j >> 1, k, t) on stream REMD_STREAM_BOOTSTRAP = 9: the 64-bit word x = (w0 << 32) | w1 for even j,
 * (w2 << 32) | w3 for odd j, selects the floor(x N_k / 2^64)-th sample of state k in ascending sample order (an exact integer high
 * multiply).  The counts are accumulated with integer atomics: exact, and free of any order.
 *
 * The drawn replicates stay on the device until the next draw.  At most REMD_MBAR_BOOTSTRAP_BATCH_ELEMENTS / N of them (and at most
 * REMD_MBAR_BOOTSTRAP_MAX_BATCH, at least 1) may be resident: 4 bytes of multiplicities and 8 of log denominator per replicate and
 * sample, 192 MiB at the bound; the partial Gram matrices of a launch are bounded by 256 MiB on top.  A host that wants more
 * replicates draws and solves them batch by batch.
 *
 * Every batched pass takes nr replicates reps[nr] of the drawn range, in any order, each at its own f_b[nr][K]; the replicate is a
 * grid dimension of its kernels.  What a pass returns for a replicate depends on (u_kn, N_k, sample_states, seed, the replicate's
 * number, its f_b) alone: not on the other replicates of the call or of the draw, and not on the run.
 * Refused, with a message: nr (or nb) < 1, a replicate outside the drawn range, a non-finite f_b, a sample_states entry that is
 * not a sampled state, a histogram of sample_states that is not N_k.                                                              */
#define REMD_MBAR_BOOTSTRAP_BATCH_ELEMENTS (1 << 24)
#define REMD_MBAR_BOOTSTRAP_MAX_BATCH 1024

/* the most replicates one draw may make resident for this problem                                                                */
int  remd_mbar_bootstrap_max_batch(remd_mbar m, int* nb);
/* draws the multiplicities of replicates b0 .. b0 + nb - 1.  sample_states[N]: the row of u_kn each sample was drawn from, or
   NULL: the samples lie in blocks, the first N_0 from state 0 and so on.                                                         */
int  remd_mbar_bootstrap_draw(remd_mbar m, uint64_t seed, const int32_t* sample_states, int b0, int nb);
/* counts[nb][N] of drawn replicates b0 .. b0 + nb - 1, for tests                                                                 */
int  remd_mbar_bootstrap_counts(remd_mbar m, int b0, int nb, uint32_t* counts);
/* log_den[nr][N] (or NULL; unchanged by the multiplicities) and phi[nr] (or NULL)                                                */
int  remd_mbar_bootstrap_log_denominator(remd_mbar m, int nr, const int32_t* reps, const double* f_b, double* log_den, double* phi);
/* one weighted application of eq. 11 to every state, sampled or not: f_new[nr][K], not shifted                                   */
int  remd_mbar_bootstrap_self_consistent(remd_mbar m, int nr, const int32_t* reps, const double* f_b, double* f_new);
/* W_sum[nr][K], gram[nr][K][K] (rows and columns of unsampled states 0; the lower triangle is computed, with c_n multiplied into
   one operand, and mirrored) and phi[nr] (or NULL)                                                                               */
int  remd_mbar_bootstrap_newton_parts(remd_mbar m, int nr, const int32_t* reps, const double* f_b, double* W_sum, double* gram, double* phi);
/* The weighted row passes of perturbed free energies and expectations.  u_ln[L][N] and A_in[I][N] are uploaded once for the call.
     f_l[nr][L]      -ln sum_n c_n exp(-u_ln - log_den_n)
     log_cA[nr][I]   ln sum_n c_n W_n,s A_in  with s = obs_state[i] < K + L a stored state (at f_b) or a perturbed one (at f_l)
   L or I may be 0 (its arrays NULL), not both.  Refused as in remd_mbar_augmented_gram, and where a perturbed state keeps no
   sample with a non-zero weight in a replicate.                                                                                  */
int  remd_mbar_bootstrap_rows(remd_mbar m, int nr, const int32_t* reps, const double* f_b, int L, const double* u_ln, int I, const double* A_in,
                              const int32_t* obs_state, double* f_l, double* log_cA);

/* ---- free energy surfaces over binned samples -----------------------------------------------------------------------------------
 * The histogram estimator of a potential of mean force (pymbar's computePMF / FES): u_n[N] is the reduced potential of every stored
 * sample at the state the surface is wanted at (+inf: the sample has weight 0), bin_n[N] its bin, -1 ... nbins - 1 (-1: in no bin).
 * With  log w_n = -u_n - log_den_n  the free energy of bin i is
 *
 *   f_i = -ln sum_{n: bin_n = i} exp(log w_n)                   (+inf for a bin without a sample of non-zero weight: it is empty)
 *
 * and its column of the weight matrix  W_n,i = exp(f_i + log w_n)  on the samples of the bin, 0 elsewhere (all 0 for an empty bin).
 * The bins are disjoint: the bin-bin block of the Gram matrix is diagonal, and neither it nor the state-bin block is formed over N.
 *
 * The host groups the samples by bin in ascending sample order (a stable counting sort) and cuts every bin's list into chunks of
 * REMD_MBAR_PMF_CHUNK samples; a workgroup reduces one chunk, reading its samples of u_kn through the list, and the chunks of a bin
 * are merged in chunk order.  No floating-point atomic: a result depends on the inputs alone, and a replicate's on no other replicate.
 * Refused, with a message: nbins outside 1 ... REMD_MBAR_PMF_MAX_BINS, a bin_n outside -1 ... nbins - 1, a NaN or -inf in u_n, a
 * non-finite f_k or f_b, N above 2^31 - 1, and for the replicates what remd_mbar_bootstrap_rows refuses.                            */
#define REMD_MBAR_PMF_MAX_BINS 65536
#define REMD_MBAR_PMF_CHUNK 256

/* the samples of one bin that one workgroup of the passes below reduces (REMD_MBAR_PMF_CHUNK), for tests and tools               */
int  remd_mbar_pmf_chunk(remd_mbar m, int64_t* chunk);
/* f_i[nbins] at f_k, and the sums the covariance needs:
     cross[K][nbins]   sum_{n in i} W_nk W_n,i                  diag[nbins]   sum_{n in i} W_n,i^2           (0 for an empty bin)
   all_parts (or NULL) [2 + K + nbins]: the column z of the normalised weight over all binned samples, W_n,z = exp(f_z + log w_n)
   with f_z = -ln sum_i exp(-f_i), from the same per-bin sums in bin order:
     [0] f_z (+inf if every bin is empty; the rest is then 0)    [1] sum_n W_n,z^2
     [2 + k] sum_n W_nk W_n,z                                    [2 + K + i] sum_n W_n,i W_n,z
   The K x K block of the Gram matrix is remd_mbar_gram's.                                                                        */
int  remd_mbar_pmf(remd_mbar m, const double* f_k, const double* u_n, const int32_t* bin_n, int nbins,
                   double* f_i, double* cross, double* diag, double* all_parts);
/* f_i[nr][nbins] = -ln sum_{n in i} c_n exp(-u_n - log_den_n) of nr drawn replicates, each with its multiplicities and its log_den at
   its f_b[nr][K] (+inf where the replicate keeps no sample of non-zero weight in the bin).  The replicate is a grid dimension; u_n and
   bin_n are uploaded once for the call.  Batching as in remd_mbar_bootstrap_rows.                                                  */
int  remd_mbar_bootstrap_pmf(remd_mbar m, int nr, const int32_t* reps, const double* f_b, const double* u_n, const int32_t* bin_n, int nbins,
                             double* f_i);

#ifdef __cplusplus
}
#endif

#endif
