/*
 * remd_hip_barostat.h — GPU-only extension of the C ABI in remd_hip.h: per-axis Monte Carlo barostats (NPγT states).
 *
 * OpenMM's MonteCarloAnisotropicBarostat and MonteCarloMembraneBarostat as the reference's ThermodynamicState accepts them
 * (openmmtools/states.py:1656): every attempt changes the volume through ONE box axis (or the xy plane), drawn among the allowed
 * ones, with a volume step adapted per axis.  The acceptance weight is
 *
 *   w = U' - U + p dV - gamma dA - N_mol kT ln(V'/V)          (dA: change of the xy area; gamma = 0 for the anisotropic kind)
 *
 * and the u_kl rows of a membrane handle carry  beta_l (U + p_l V - gamma_l A_xy).  remd_set_barostat (remd_hip.h) is the isotropic
 * barostat and is unchanged; the last of the two calls decides which move a handle makes.  remd_barostat_attempts, remd_get_boxes,
 * the in-integrator slot (every `frequency`-th step), the restart attempts and the refusal of a box below twice the cutoff work in
 * both modes.
 *
 * These entry points are declared here and not in remd_hip.h because the CPU port of the ABI does not provide them: a host binds
 * them only where the loaded library exports them.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_BAROSTAT_H
#define REMD_HIP_BAROSTAT_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REMD_BAROSTAT_ANISOTROPIC 1
#define REMD_BAROSTAT_MEMBRANE    2

/* MonteCarloMembraneBarostat's modes */
#define REMD_BAROSTAT_XY_ISOTROPIC    0
#define REMD_BAROSTAT_XY_ANISOTROPIC  1
#define REMD_BAROSTAT_Z_FREE          0
#define REMD_BAROSTAT_Z_FIXED         1
#define REMD_BAROSTAT_CONSTANT_VOLUME 2

/* pressure[K] in kJ/mol/nm^3 and surface_tension[K] in kJ/mol/nm^2 (bar nm x 0.06022140857) per state, K as in remd_set_states
   (call after it).  kind = REMD_BAROSTAT_ANISOTROPIC: xy_or_scale_mask = scaleX | scaleY << 1 | scaleZ << 2 (at least one bit),
   surface_tension and zmode are ignored.  kind = REMD_BAROSTAT_MEMBRANE: xy_or_scale_mask = the xy mode, zmode the z mode,
   surface_tension = NULL means 0.  pressure = NULL or frequency <= 0 switches the barostat off, as in remd_set_barostat.          */
int  remd_set_barostat_axes(remd_handle h, int K, const double* pressure, const double* surface_tension,
                            int kind, int xy_or_scale_mask, int zmode, int frequency);
/* per local replica and axis (x, y, z): the volume step (nm^3) and the totals of attempted and accepted moves.  A membrane
   barostat with the isotropic xy mode counts its xy moves under x.  Any pointer may be NULL.                                      */
int  remd_get_barostat_axis_stats(remd_handle h, double* volume_scale /*[R][3]*/, int64_t* n_attempted /*[R][3]*/,
                                  int64_t* n_accepted /*[R][3]*/);

#ifdef __cplusplus
}
#endif

#endif
