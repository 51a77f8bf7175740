/*
 * remd_hip_vsites.h — GPU-only extension of the C ABI in remd_hip.h: virtual sites (four- and five-site waters, lone pairs).
 *
 * A virtual site is a massless particle whose position is a fixed function of two or three parent particles (OpenMM's
 * TwoParticleAverageSite, ThreeParticleAverageSite and OutOfPlaneSite, with OpenMM's definitions):
 *
 *   averages:      x = sum_i w_i x_i
 *   out of plane:  x = x1 + w12 r12 + w13 r13 + wcross (r12 x r13),   r12 = x2 - x1, r13 = x3 - x1
 *
 * The differences are plain (no minimum image): the parents of a site lie in one molecule, which the engine keeps whole.  The
 * engine places every site from its parents in front of each force evaluation and behind every call that moves positions, and
 * hands the force on a site to its parents by the chain rule before anything reads the forces; remd_get_forces returns zero on
 * the sites.  A site is no degree of freedom: it is never kicked, gets no noise, and keeps velocity zero.
 *
 * remd_set_system accepts a particle of mass exactly 0 only as a site to be: until remd_set_virtual_sites has declared every
 * massless particle, remd_set_replicas refuses the handle ("massless particles are not supported").  remd_set_system forgets the
 * sites of the system before.
 *
 * Declared here and not in remd_hip.h because the CPU port of the ABI does not provide it: a host binds the entry point only
 * where the loaded library exports it.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_VSITES_H
#define REMD_HIP_VSITES_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REMD_VSITE_TWO_AVERAGE   0     /* parent[0 .. 1], weight = w1, w2                 */
#define REMD_VSITE_THREE_AVERAGE 1     /* parent[0 .. 2], weight = w1, w2, w3             */
#define REMD_VSITE_OUT_OF_PLANE  2     /* parent[0 .. 2], weight = w12, w13, wcross       */

typedef struct remd_vsite_desc {
    int32_t kind;                      /* REMD_VSITE_*                                                    */
    int32_t site;                      /* the particle that is placed: mass 0 in the system descriptor    */
    int32_t parent[3];                 /* distinct particles with mass, none of them a site; unused: -1   */
    double  weight[3];
} remd_vsite_desc;

/* After remd_set_system.  Refused with the handle as it was: an index out of range, a parent named twice, a parent that is a
   site or massless, a site with mass, a site named twice, an unknown kind, a weight that is not finite.  n = 0 drops the table. */
int  remd_set_virtual_sites(remd_handle h, const remd_vsite_desc* sites, int32_t n);

#ifdef __cplusplus
}
#endif

#endif
