/*
 * remd_hip_timeseries.h — GPU-only extension of the C ABI in remd_hip.h: the statistical inefficiency of the suffixes of a
 * timeseries on the device.
 *
 * The automated equilibration detection of Chodera (JCTC 12, 1799 (2016)) as multistate/analysis.py runs it asks for the
 * statistical inefficiency g (Chodera et al., JCTC 3, 26 (2007)) of the suffix A[t_s:] at many time origins t_s.  With
 * N_s = N - t_s, mean and sigma2 = mean (A - mean)^2 taken over the suffix, and dA = A - mean:
 *
 *   C(t) = sum_{n = t_s}^{N - t - 1} dA_n dA_{n+t} / ((N_s - t) sigma2)
 *   g    = 1 + sum_t 2 C(t) (1 - t / N_s) increment(t)             over the lags t = 1, 2, 3, ... (increment 1), or with `fast`
 *                                                                   t = 1, 2, 4, 7, 11, ... (the increment grows by 1 per lag)
 *
 * summed until the first C(t) <= 0 at a lag t > mintime, or until t >= N_s - 1; the result is max(g, 1).  This is
 * analysis.statistical_inefficiency, lag for lag.  Everything is f64.  No pass uses a floating-point atomic: every sum is taken
 * per chunk of samples, the chunks are cut at absolute sample indices and merged in chunk order, so a result depends on A, the
 * origin and the lag alone: not on the other origins of the call, nor on how the lags were batched.
 *
 * A timeseries is an object of its own: it needs a device, not a remd_handle.  A failed call returns non-zero and leaves its
 * message in remd_last_error(NULL).
 *
 * These entry points are declared here and not in remd_hip.h because the CPU port of the ABI does not provide them: a host binds
 * them only where the loaded library exports them.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_TIMESERIES_H
#define REMD_HIP_TIMESERIES_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most lags of one batch: the host enqueues batches of 8, 16, 32, then 64 lags until every origin has stopped */
#define REMD_TIMESERIES_MAX_BATCH 64

typedef struct remd_timeseries_ctx* remd_timeseries;

/* Uploads A[N] once.  Refused: N < 2, a non-finite sample.                                                                        */
int  remd_timeseries_create(int device, int64_t N, const double* A, remd_timeseries* out);
void remd_timeseries_destroy(remd_timeseries ts);

/* g[S] of the suffixes A[origin[s]:], 0 <= origin[s] <= N - 2 (any order, repeats allowed); fast != 0: the growing increments.
   status[S]: 0, or 1 for a suffix with sigma2 == 0, whose g is NaN (the host function raises there).  last_lag[S] (or NULL): the
   last lag whose term was added to g, 0 if none was.  Refused: an origin out of range, S < 1, mintime < 0.                         */
int  remd_timeseries_inefficiency(remd_timeseries ts, int32_t S, const int64_t* origin, int fast, int mintime, double* g,
                                  int32_t* status, int64_t* last_lag);
/* the samples per workgroup of every pass (chunk c covers the samples [c * chunk, (c + 1) * chunk)), for tests and tools         */
int  remd_timeseries_chunks(remd_timeseries ts, int64_t* chunk);
/* device milliseconds of the kernels of the last remd_timeseries_inefficiency on this object (events around the launches of each
   batch, summed; the read-backs between batches are not in it), for tools                                                         */
int  remd_timeseries_last_ms(remd_timeseries ts, double* ms);

#ifdef __cplusplus
}
#endif

#endif
