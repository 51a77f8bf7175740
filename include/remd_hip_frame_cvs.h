/*
 * remd_hip_frame_cvs.h — GPU-only extension of the C ABI in remd_hip.h: collective variables of stored frames.
 *
 * The coordinates a free energy surface is taken over (multistate/analysis.py: get_collective_variables -> get_pmf), evaluated at F
 * stored frames with the conventions of the force kernels, so that a surface is over the variable the run was biased along:
 *
 *   centroid   c = x_first + sum_i w_i img(x_i - x_first), the w_i normalised; img the minimum image under the frame's own box when
 *              the variable is periodic and a box is given (centroid_sum.h, the convention of remd_restraint_frames)
 *   distance   |d|, d = img(c2 - c1)
 *   angle      acos of the cosine of img(c1 - c2) and img(c3 - c2), clamped to [-1, 1]
 *   dihedral   atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3)), b_k = img(c_k+1 - c_k): sign and range (-pi, pi] of PeriodicTorsionForce
 *   RMSD       system.RMSDForce's (custom_cv.hip): positions relative to the first particle, the reference centred by the caller, the
 *              rotation of custom_cv_math.h, the deviation summed directly; a mean square deviation below 1e-20 nm^2 gives 0.  No
 *              minimum images: the particles must belong to one molecule.
 *
 * Everything is f64 from the f32 positions.  No floating-point atomic: every sum is taken in a fixed order that depends on the
 * variable alone, so a value is bit-identical from run to run and depends neither on the chunking nor on the other variables of the call.
 *
 * This entry point is declared here and not in remd_hip.h because the CPU port of the ABI does not provide it: a host binds
 * it only where the loaded library exports it.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_FRAME_CVS_H
#define REMD_HIP_FRAME_CVS_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REMD_FRAME_CV_DISTANCE 0   /* 2 groups */
#define REMD_FRAME_CV_ANGLE    1   /* 3 groups */
#define REMD_FRAME_CV_DIHEDRAL 2   /* 4 groups */
#define REMD_FRAME_CV_RMSD     3   /* 1 group  */

/* The variables as CSR tables.  Variable v is of kind[v] (REMD_FRAME_CV_*) and periodic[v] (0 / 1; not read for an RMSD); its groups
   are cv_groups[v] ... cv_groups[v + 1] - 1, as many as its kind takes; group g holds the entries group_off[g] ... group_off[g + 1] - 1
   of atoms (indices into 0 ... n_atoms-1) and weights (normalised: every group's sum to 1; an RMSD's are not read).  reference
   [entries][3]: for the entries of an RMSD's group, the reference positions centred on their own centroid; not read elsewhere (NULL
   without an RMSD).                                                                                                                */
typedef struct remd_frame_cv_tables {
    int32_t n_cv;
    const int32_t* kind;           /* [n_cv]                      */
    const int32_t* periodic;       /* [n_cv]                      */
    const int32_t* cv_groups;      /* [n_cv + 1]                  */
    const int32_t* group_off;      /* [cv_groups[n_cv] + 1]       */
    const int32_t* atoms;          /* [group_off[last]]           */
    const double* weights;         /* [group_off[last]]           */
    const double* reference;       /* [group_off[last]][3] / NULL */
} remd_frame_cv_tables;

/* out[F][n_cv] (nm, rad) of the variables at F stored frames.  No handle: a device (like remd_restraint_frames).
   pos [F][n_atoms][3] f32, box [F][3] f32 (NULL: no variable takes minimum images, whatever periodic[] says; the caller decides whether
   that is an error).  max_frames_per_launch <= 0: the library's choice.  The host uploads at most that many frames at a time; a
   frame's result does not depend on the chunking.  kernel_ms (or NULL): device milliseconds (events) of the kernels of this call.
   Refused before anything is launched (non-zero, the reason in remd_last_error(NULL)): F < 1, n_atoms < 1, no variable, NULL tables,
   pos or out, an unknown kind, offsets that do not ascend from 0 or a variable with another number of groups than its kind takes, an
   empty group, fewer than 3 particles in an RMSD, an atom index outside 0 ... n_atoms-1, a non-finite or negative weight or weights
   that do not sum to 1 within 1e-9, an RMSD without reference or with a non-finite one, a non-finite or non-positive edge in box.    */
int  remd_frame_cvs(int device, int64_t F, int n_atoms, const float* pos, const float* box, const remd_frame_cv_tables* tables,
                    int64_t max_frames_per_launch, double* out, double* kernel_ms);

#ifdef __cplusplus
}
#endif

#endif
