/*
 * remd_hip_gb.h — GPU-only extension of the C ABI in remd_hip.h: the constants and the cutoff of the implicit-solvent model.
 *
 * remd_set_gbsa (remd_hip.h) evaluates OBC2 without a cutoff.  A CustomGBForce of the OBC family (openmmtools_amd/custom_gb.py
 * recognises it) has free constants:
 *
 *   I_i = sum_{j != i, r_ij < cutoff} s_j H(r_ij; R_i - offset, scale_j (R_j - offset))
 *   B_i = 1 / (1 / (R_i - offset) - tanh(alpha psi - beta psi^2 + gamma psi^3) / R_i),   psi = I_i (R_i - offset)
 *   E   = sum_i s_i [surface (R_i + probe)^2 (R_i / B_i)^6 - k_e tau q_i^2 / (2 B_i)]
 *         - sum_{i<j, r_ij < cutoff} k_e tau s_i q_i s_j q_j / sqrt(r^2 + B_i B_j exp(-r^2 / (4 B_i B_j)))
 *
 * (surface multiplies the surface term only where remd_gbsa_desc.surface_area is 1).  REMD_GB_CUTOFF_PERIODIC is OpenMM's
 * CustomGBForce::CutoffPeriodic: r_ij is the minimum image under each replica's own box, the pair sums see only pairs with r < cutoff,
 * with no shift and no switching; the single-particle terms are unchanged.  It needs a periodic system (CutoffPeriodic or PME
 * NonbondedForce) and a cutoff of at most half the shortest box edge.  REMD_GB_NO_CUTOFF needs a NoCutoff system.
 *
 * These entry points are declared here and not in remd_hip.h because the CPU port of the ABI does not provide them: a host binds
 * them only where the loaded library exports it.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_GB_H
#define REMD_HIP_GB_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REMD_GB_NO_CUTOFF       0
#define REMD_GB_CUTOFF_PERIODIC 2

typedef struct remd_gb_model_desc {
    double offset, alpha, beta, gamma, ke, surface, probe;   /* nm, -, -, -, kJ nm/mol/e^2, kJ/mol/nm^2, nm        */
    int32_t method;                                          /* REMD_GB_NO_CUTOFF or REMD_GB_CUTOFF_PERIODIC       */
    double cutoff;                                           /* nm (REMD_GB_CUTOFF_PERIODIC)                       */
} remd_gb_model_desc;

/* the model of the handle's implicit solvent; call after remd_set_gbsa (which resets it to OBC2 without a cutoff).  m = NULL: OBC2,
   NoCutoff (offset 0.009, alpha 1, beta 0.8, gamma 4.85, k_e 138.935485, surface 28.3919551, probe 0.14).                        */
int  remd_set_gb_model(remd_handle h, const remd_gb_model_desc* m);

#ifdef __cplusplus
}
#endif

#endif
