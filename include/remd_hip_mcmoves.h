/*
 * remd_hip_mcmoves.h — GPU-only extension of the C ABI in remd_hip.h: Metropolized rigid-body Monte Carlo moves.
 *
 * The reference's MCDisplacementMove and MCRotationMove (mcmc.py:1704-1910) for all local replicas at once, without the host:
 * a subset of atoms is translated by one normal vector, or rotated about its centre of geometry by a uniformly random rotation
 * (Shoemake's quaternion, the reference's matrix), and the proposal is accepted with min(1, exp(-beta (U' - U))) at the replica's
 * own state; a rejected replica gets the subset's positions, its forces and its potential back to the bit.  The volume does not
 * change, so neither a p V term nor the per-state long-range constant enters the test.
 *
 * Random numbers: the stream REMD_STREAM_MC_MOVE (8) of csrc/rng.h, counter
 *   a = 4 * position + block,   b = global replica (remd_set_replica_ids where set, else r_begin + r),   t = iteration.
 * Blocks 0 and 1 give four uniforms u0 = u53(w0, w1), u1 = u53(w2, w3) (block 0), u2, u3 likewise (block 1); block 2 gives the
 * acceptance uniform u53(w2, w3).
 *   displacement:  sigma sqrt(-2 ln(1 - u0)) (cos, sin)(2 pi u1) for x and y,  sigma sqrt(-2 ln(1 - u2)) cos(2 pi u3) for z;
 *   rotation:      q = (sqrt(1 - u0) sin 2 pi u1, sqrt(1 - u0) cos 2 pi u1, sqrt(u0) sin 2 pi u2, sqrt(u0) cos 2 pi u2).
 * A run is reproducible and does not depend on how the replicas are sharded over ranks or handles.
 *
 * Declared here and not in remd_hip.h because the CPU port of the ABI does not provide it: a host binds the entry point only
 * where the loaded library exports it.  Conventions as in remd_hip.h.
 */
#ifndef REMD_HIP_MCMOVES_H
#define REMD_HIP_MCMOVES_H

#include "remd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REMD_MC_DISPLACEMENT 0
#define REMD_MC_ROTATION     1
#define REMD_MC_MAX_MOVES    16

typedef struct remd_mc_move_desc {
    int32_t kind;                      /* REMD_MC_DISPLACEMENT or REMD_MC_ROTATION                              */
    int32_t n_atoms;
    const int32_t* atoms;              /* [n_atoms] the subset: distinct, in any order, not necessarily contiguous */
    double  sigma_nm;                  /* standard deviation per axis of the displacement (ignored by a rotation) */
    int32_t position;                  /* place of the move in the flattened sequence: keys its random numbers    */
} remd_mc_move_desc;

/* The moves in order, each for all local replicas at once; one host synchronisation, at the end.  accepted[m * R_local + r] is
   1 where replica r accepted move m, else 0.  Afterwards the forces the handle holds belong to the positions it holds.
   Refused with the handle as it was: replicas not set, n_moves outside 1 .. REMD_MC_MAX_MOVES, an unknown kind, n_atoms < 1, an
   atom index out of range or named twice, a negative or non-finite sigma, a negative position. */
int  remd_mc_rigid_moves(remd_handle h, const remd_mc_move_desc* moves, int32_t n_moves, int64_t iteration,
                         int32_t* accepted /*[n_moves][R_local]*/);

#ifdef __cplusplus
}
#endif

#endif
