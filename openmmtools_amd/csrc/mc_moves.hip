// Metropolized rigid-body Monte Carlo moves (include/remd_hip_mcmoves.h): the reference's MCDisplacementMove and MCRotationMove
// (mcmc.py:1704-1910) for all local replicas at once, shaped like the barostat attempt (barostat.hip): evaluate, move, evaluate,
// decide, restore, all on the handle's stream.  Per move three small launches beside the evaluations:
//   mc_propose_kernel   one workgroup per replica: the replica's draws, the subset's old positions copied aside, the new ones
//                       computed in f64 from the f32 positions and stored rounded once;
//   mc_decide_kernel    one lane per replica: accept when delta <= 0 or u < exp(-delta), delta = beta[label] (U' - U);
//   mc_restore_kernel   rejected replicas only: the subset's positions, every force word and the potential back from the copies.
// The copies live in the barostat's save buffers (the two never overlap in time).  No floating-point atomics anywhere: the centre
// of geometry is a sum in a fixed order, so a run gives the same bits every time and on every sharding of the replicas.
#include "remd_internal.h"
#include "rng.h"
#include "../../include/remd_hip_mcmoves.h"
#include <cmath>

#define MC_BLOCK 256          // lanes of a propose workgroup (tests/test_mc_moves_device_gpu.py moves MC_BLOCK + 1 atoms)

struct mc_draws { double u0, u1, u2, u3; };

__device__ __forceinline__ mc_draws mc_uniforms(uint64_t seed, int position, uint32_t replica, long long iteration)
{
    const philox4 a = remd_philox(seed, REMD_STREAM_MC_MOVE, 4u * (uint32_t)position, replica, (uint64_t)iteration);
    const philox4 b = remd_philox(seed, REMD_STREAM_MC_MOVE, 4u * (uint32_t)position + 1u, replica, (uint64_t)iteration);
    return mc_draws{ remd_u53(a.w[0], a.w[1]), remd_u53(a.w[2], a.w[3]), remd_u53(b.w[0], b.w[1]), remd_u53(b.w[2], b.w[3]) };
}

__global__ __launch_bounds__(MC_BLOCK)
void mc_propose_kernel(int kind, int n_atoms, const int* __restrict__ atoms, double sigma, int position, int r_begin, uint64_t seed,
                       long long iteration, const unsigned int* __restrict__ noise_id, int Npad, float4* __restrict__ pos,
                       float4* __restrict__ x0)
{
    __shared__ double part[3][MC_BLOCK];
    const int r = blockIdx.x, t = threadIdx.x;
    float4* P = pos + (size_t)r * Npad;
    float4* S = x0 + (size_t)r * Npad;
    // every lane computes the replica's draws itself: the same integer and f64 arithmetic in every lane, nothing to hand round
    const mc_draws u = mc_uniforms(seed, position, noise_id ? noise_id[r] : (uint32_t)(r_begin + r), iteration);
    if (kind == REMD_MC_DISPLACEMENT) {
        // Box-Muller (sin and cos of 2 pi u as sincospi(2 u): the argument is reduced exactly)
        double s1, c1, s3, c3;
        sincospi(2.0 * u.u1, &s1, &c1);
        sincospi(2.0 * u.u3, &s3, &c3);
        const double rxy = sigma * sqrt(-2.0 * log(1.0 - u.u0)), rz = sigma * sqrt(-2.0 * log(1.0 - u.u2));
        const double dx = rxy * c1, dy = rxy * s1, dz = rz * c3;
        for (int k = t; k < n_atoms; k += MC_BLOCK) {
            const int a = atoms[k];
            const float4 p = P[a];
            S[a] = p;
            P[a] = make_float4((float)((double)p.x + dx), (float)((double)p.y + dy), (float)((double)p.z + dz), p.w);
        }
        return;
    }
    // centre of geometry: per-lane strided partial sums, then a fixed tree -- the order of the additions is a function of
    // (n_atoms, MC_BLOCK) alone
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = t; k < n_atoms; k += MC_BLOCK) {
        const float4 p = P[atoms[k]];
        sx += (double)p.x; sy += (double)p.y; sz += (double)p.z;
    }
    part[0][t] = sx; part[1][t] = sy; part[2][t] = sz;
    __syncthreads();
    for (int w = MC_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) { part[0][t] += part[0][t + w]; part[1][t] += part[1][t + w]; part[2][t] += part[2][t + w]; }
        __syncthreads();
    }
    const double cx = part[0][0] / (double)n_atoms, cy = part[1][0] / (double)n_atoms, cz = part[2][0] / (double)n_atoms;
    // Shoemake's uniform quaternion and the reference's matrix of it (mcmc.py:1842-1906; the quaternion need not be normalised)
    double s1, c1, s2, c2;
    sincospi(2.0 * u.u1, &s1, &c1);
    sincospi(2.0 * u.u2, &s2, &c2);
    const double ra = sqrt(1.0 - u.u0), rb = sqrt(u.u0);
    const double qw = ra * s1, qx = ra * c1, qy = rb * s2, qz = rb * c2;
    const double n = qw * qw + qx * qx + qy * qy + qz * qz;
    const double s = n > 0.0 ? 2.0 / n : 0.0;
    const double m00 = 1.0 - s * (qy * qy + qz * qz), m01 = s * (qx * qy - qw * qz), m02 = s * (qx * qz + qw * qy);
    const double m10 = s * (qx * qy + qw * qz), m11 = 1.0 - s * (qx * qx + qz * qz), m12 = s * (qy * qz - qw * qx);
    const double m20 = s * (qx * qz - qw * qy), m21 = s * (qy * qz + qw * qx), m22 = 1.0 - s * (qx * qx + qy * qy);
    for (int k = t; k < n_atoms; k += MC_BLOCK) {
        const int a = atoms[k];
        const float4 p = P[a];
        S[a] = p;
        const double x = (double)p.x - cx, y = (double)p.y - cy, z = (double)p.z - cz;
        P[a] = make_float4((float)(m00 * x + m01 * y + m02 * z + cx), (float)(m10 * x + m11 * y + m12 * z + cy),
                           (float)(m20 * x + m21 * y + m22 * z + cz), p.w);
    }
}

// The volume does not change under a rigid move of a subset, so neither p V nor the per-state long-range constant (~ 1/V, which
// d_potential does not carry) enters: delta is beta times the difference of the two potentials and nothing else.
__global__ void mc_decide_kernel(int R, int r_begin, uint64_t seed, long long iteration, int position, const double* __restrict__ U_old,
                                 const double* __restrict__ U_new, const int64_t* __restrict__ labels, const double* __restrict__ beta,
                                 const unsigned int* __restrict__ noise_id, int* __restrict__ accepted)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const double delta = beta[labels[r_begin + r]] * (U_new[r] - U_old[r]);
    const philox4 q = remd_philox(seed, REMD_STREAM_MC_MOVE, 4u * (uint32_t)position + 2u, noise_id ? noise_id[r] : (uint32_t)(r_begin + r),
                                  (uint64_t)iteration);
    accepted[r] = (delta <= 0.0 || remd_u53(q.w[2], q.w[3]) < exp(-delta)) ? 1 : 0;       // a NaN on either side rejects
}

__global__ __launch_bounds__(256)
void mc_restore_kernel(int N, int Npad, int n_atoms, const int* __restrict__ atoms, const int* __restrict__ accepted,
                       float4* __restrict__ pos, const float4* __restrict__ x0, long long* __restrict__ force,
                       const long long* __restrict__ f0, double* __restrict__ potential, const double* __restrict__ U0)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (accepted[r]) return;
    if (i == 0) potential[r] = U0[r];
    if (i >= N) return;
    const size_t o = (size_t)r * Npad, of = (size_t)r * 3 * Npad;
    if (i < n_atoms) { const int a = atoms[i]; pos[o + a] = x0[o + a]; }          // (n_atoms <= N: the subset's atoms are distinct)
    force[of + i] = f0[of + i]; force[of + Npad + i] = f0[of + Npad + i]; force[of + 2 * Npad + i] = f0[of + 2 * Npad + i];
}

// what the kernels index unchecked is checked here; nothing of the handle has changed when a description is refused
static int mc_check(remd_ctx* h, const remd_mc_move_desc* moves, int n_moves, std::vector<int>& flat, std::vector<int>& first)
{
    if (n_moves < 1 || n_moves > REMD_MC_MAX_MOVES) return remd_fail(h, -1, "remd_mc_rigid_moves: n_moves must be 1 .. 16");
    std::vector<char> seen((size_t)h->N);
    for (int m = 0; m < n_moves; ++m) {
        const remd_mc_move_desc& d = moves[m];
        if (d.kind != REMD_MC_DISPLACEMENT && d.kind != REMD_MC_ROTATION) return remd_fail(h, -3, "remd_mc_rigid_moves: unknown kind of move");
        if (d.n_atoms < 1 || !d.atoms) return remd_fail(h, -3, "remd_mc_rigid_moves: a move needs at least one atom");
        if (d.kind == REMD_MC_DISPLACEMENT && !(std::isfinite(d.sigma_nm) && d.sigma_nm >= 0.0))
            return remd_fail(h, -3, "remd_mc_rigid_moves: sigma must be finite and not negative");
        if (d.position < 0 || d.position >= (1 << 29)) return remd_fail(h, -3, "remd_mc_rigid_moves: position out of range");
        std::fill(seen.begin(), seen.end(), 0);
        first.push_back((int)flat.size());
        for (int k = 0; k < d.n_atoms; ++k) {
            const int a = d.atoms[k];
            if (a < 0 || a >= h->N) return remd_fail(h, -3, "remd_mc_rigid_moves: atom index out of range");
            if (seen[a]) return remd_fail(h, -3, "remd_mc_rigid_moves: an atom is named twice");
            seen[a] = 1;
            flat.push_back(a);
        }
    }
    return 0;
}

int remd_mc_moves_enqueue(remd_ctx* h, const remd_mc_move_desc* moves, int n_moves, int64_t iteration)
{
    std::vector<int> flat, first;
    int rc;
    if ((rc = mc_check(h, moves, n_moves, flat, first))) return rc;
    const int R = h->R, Npad = h->Npad;
    if ((rc = remd_barostat_buffers(h))) return rc;                    // the save buffers, shared with the barostat
    if (flat != h->mc_atoms_host) {                                     // the subsets of a sampler's sequence: uploaded once
        REMD_CHECK(h, hipStreamSynchronize(h->stream));
        REMD_TRY(h->d_mc_atoms.upload(h, flat));
        h->mc_atoms_host = flat;
    }
    REMD_TRY(h->d_mc_acc.grow(h, (size_t)REMD_MC_MAX_MOVES * R));
    for (int m = 0; m < n_moves; ++m) {
        const remd_mc_move_desc& d = moves[m];
        const int* d_atoms = h->d_mc_atoms + first[m];
        int* d_acc = h->d_mc_acc + (size_t)m * R;
        if (m == 0) {
            // U and the forces of the current configuration.  Behind an earlier move of this call they are already there: accepted
            // replicas hold those of the proposal they took, rejected ones got theirs back
            h->force_zeroed = false;
            if ((rc = remd_compute_forces(h, true))) return rc;
        }
        REMD_CHECK(h, hipMemcpyAsync(h->d_baro_U0, h->d_potential, sizeof(double) * R, hipMemcpyDeviceToDevice, h->stream));
        REMD_CHECK(h, hipMemcpyAsync(h->d_baro_f0, h->d_force, sizeof(long long) * 3 * (size_t)R * Npad, hipMemcpyDeviceToDevice, h->stream));
        {
            remd_prof_scope ps(h, "mc_propose");
            hipLaunchKernelGGL(mc_propose_kernel, dim3(R), dim3(MC_BLOCK), 0, h->stream, d.kind, d.n_atoms, d_atoms, d.sigma_nm, d.position,
                               h->r_begin, h->seed, (long long)iteration, h->d_noise_id, Npad, h->d_pos, h->d_baro_x0);
        }
        // U' and the forces of the proposal (the evaluation places the virtual sites of the moved parents in front of everything else)
        h->force_zeroed = false;
        if ((rc = remd_compute_forces(h, true))) return rc;
        {
            remd_prof_scope ps(h, "mc_decide");
            hipLaunchKernelGGL(mc_decide_kernel, dim3((R + 63) / 64), dim3(64), 0, h->stream, R, h->r_begin, h->seed, (long long)iteration,
                               d.position, h->d_baro_U0, h->d_potential, h->d_labels, h->d_beta, h->d_noise_id, d_acc);
            hipLaunchKernelGGL(mc_restore_kernel, dim3((h->N + 255) / 256, R), dim3(256), 0, h->stream, h->N, Npad, d.n_atoms, d_atoms, d_acc,
                               h->d_pos, h->d_baro_x0, h->d_force, h->d_baro_f0, h->d_potential, h->d_baro_U0);
        }
        REMD_TRY(remd_vsites_place(h, h->stream));                      // sites of parents that went back (nothing without sites)
        h->forces_valid = true; h->force_zeroed = false;
    }
    REMD_CHECK(h, hipGetLastError());
    return 0;
}
