/*
 * remd_hip_restraints.h — GPU-only extension of the C ABI in remd_hip.h: receptor-ligand restraints.
 *
 * The radially symmetric restraints of openmmtools/forces.py (HarmonicRestraintForce, FlatBottomRestraintForce and their
 * *BondForce variants): an energy of the distance r between the mass-weighted centroids of two groups of atoms,
 *
 *   harmonic     E = lambda * (K/2) r^2
 *   flat bottom  E = lambda * step(r - r0) (K/2) (r - r0)^2
 *
 * lambda being the value of the force's controlling global parameter (lambda_restraints) at the replica's state.  A restraint acts
 * in every force evaluation (MD steps, energies, the barostat, minimisation) and in the u_kl rows: column l of replica r adds
 * beta_l (lambda_l - lambda_own(r)) E_r, E_r the unscaled energy at the replica's positions.
 *
 * These entry points are declared here and not in remd_hip.h because the CPU port of the ABI does not provide them: a host binds
 * them only where the loaded library exports them.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_RESTRAINTS_H
#define REMD_HIP_RESTRAINTS_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REMD_RESTRAINT_HARMONIC    0
#define REMD_RESTRAINT_FLAT_BOTTOM 1

typedef struct remd_restraint_desc {
    int32_t kind;                  /* REMD_RESTRAINT_*                                                                    */
    double K;                      /* kJ/mol/nm^2                                                                         */
    double r0;                     /* nm (flat bottom; ignored by the harmonic form)                                      */
    int32_t n1; const int32_t* atoms1; const double* weights1;   /* group 1: atoms and centroid weights (NULL: masses)   */
    int32_t n2; const int32_t* atoms2; const double* weights2;   /* group 2                                              */
    int32_t periodic;              /* 1: the centroid difference is the minimum image under the replica's own box         */
    int32_t force_group;           /* Force.getForceGroup() (multiple-time-step splittings)                              */
} remd_restraint_desc;

/* the restraints of the system; call after remd_set_system (which forgets them).  n = 0: none.  Every restraint of a handle sits in
   one force group.  Every state's lambda starts at 1 until remd_set_restraint_lambdas.                                           */
int  remd_set_restraints(remd_handle h, const remd_restraint_desc* desc, int n);
/* lambda[K][n]: every state's value of each restraint's controlling parameter; K as in remd_set_states (call after it)          */
int  remd_set_restraint_lambdas(remd_handle h, const double* lambda);
/* out[R_local][n]: the unscaled restraint energies (kJ/mol) at the local replicas' current positions                            */
int  remd_get_restraint_energies(remd_handle h, double* out);

/* ---- the analysis pass over stored frames: no handle, a device (like the entry points of remd_hip_mbar.h) ----------------------
   energy[F] (kJ/mol, unscaled: lambda = 1) and distance[F] (nm; either may be NULL) of one restraint at F stored frames.
   pos [F][n_atoms][3] f32, box [F][3] f32 (NULL: not periodic; required when desc->periodic).
   desc's atom indices address 0 ... n_atoms-1; weights NULL -> masses[n_atoms].  desc->force_group is not read.
   max_frames_per_launch <= 0: the library's choice.  The host uploads at most that many frames at a time; a frame's result does
   not depend on the chunking.  The centroid is the engine's own, the one the run was sampled with: first atom + sum_i w_i
   img(x_i - x_first), img the minimum image under the frame's own box when periodic, in f64 in a fixed order.
   Refused before anything is launched (non-zero, the reason in remd_last_error(NULL)): F < 1, an empty group, an atom index outside
   0 ... n_atoms-1, a negative weight or weights that sum to zero, periodic without box, a non-finite or non-positive box edge when
   periodic, an unknown kind, K or r0 < 0, a NULL desc or pos.                                                                       */
int  remd_restraint_frames(int device, const remd_restraint_desc* desc, int64_t F, int n_atoms,
                           const float* pos, const float* box, const double* masses,
                           int64_t max_frames_per_launch, double* energy, double* distance);
/* device milliseconds (events) of the kernels of the last completed remd_restraint_frames call of this process                   */
int  remd_restraint_frames_last_ms(double* ms);

#ifdef __cplusplus
}
#endif

#endif
