#include "remd_internal.h"
#include "rng.h"
#include "../../include/remd_hip_barostat.h"
#include <cmath>

// Monte Carlo barostat: what an NPT ThermodynamicState means in the reference (states.py:1177-1181 adds an
// openmm.MonteCarloBarostat, frequency 25, to the System; it fires inside LangevinIntegrator's addUpdateContextState step,
// integrators.py:1313).  The algorithm is OpenMM's MonteCarloBarostatImpl::updateContextState, restated: every
// `frequency` steps  dV = volumeScale * 2 (u - 1/2);  every molecule's centre (arithmetic mean, wrapped into the box) is
// scaled by s = (V'/V)^(1/3) together with the box;  w = U' - U + p dV - N_mol kT ln(V'/V);  reject (restore) if w > 0 and
// u' > exp(-w / kT);  after >= 10 attempts volumeScale /= 1.1 below 25 % acceptance, *= 1.1 (capped at 0.3 V) above 75 %.
// All local replicas attempt at once, each with its own state's p and kT and its own Philox draws.
__global__ void baro_draw_kernel(int R, int r_begin, uint64_t seed, long long attempt, float* __restrict__ box,
                                 float* __restrict__ box_old, double* __restrict__ st, const unsigned int* __restrict__ noise_id)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double* S = st + (size_t)r * 8;
    const double Lx = box[4 * r], Ly = box[4 * r + 1], Lz = box[4 * r + 2];
    const double V = Lx * Ly * Lz;
    if (S[0] <= 0.0) S[0] = 0.01 * V;                                   // initial volumeScale (MonteCarloBarostatImpl::initialize)
    const philox4 w = remd_philox(seed, REMD_STREAM_BAROSTAT, 0u, noise_id ? noise_id[r] : (uint32_t)(r_begin + r), (uint64_t)attempt);
    const double dV = S[0] * 2.0 * (remd_u53(w.w[2], w.w[3]) - 0.5);
    const double newV = V + dV;
    const double scale = cbrt(newV / V);
    S[5] = dV; S[6] = newV; S[7] = V;
    box_old[4 * r] = box[4 * r]; box_old[4 * r + 1] = box[4 * r + 1]; box_old[4 * r + 2] = box[4 * r + 2];
    box[4 * r] = (float)(Lx * scale); box[4 * r + 1] = (float)(Ly * scale); box[4 * r + 2] = (float)(Lz * scale);
}

// one thread per molecule (contiguous atom range): centre -> wrapped centre -> scaled centre (OpenMM scalePositions)
__global__ __launch_bounds__(256)
void baro_scale_kernel(int n_mol, const int* __restrict__ first, const int* __restrict__ size, int Npad,
                       float4* __restrict__ pos, const float* __restrict__ box_old, const double* __restrict__ st)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (g >= n_mol) return;
    const double* S = st + (size_t)r * 8;
    const float scale = (float)cbrt(S[6] / S[7]);
    float4* P = pos + (size_t)r * Npad;
    const int a0 = first[g], n = size[g];
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int k = 0; k < n; ++k) { const float4 p = P[a0 + k]; cx += p.x; cy += p.y; cz += p.z; }
    const float inv = 1.f / (float)n;
    cx *= inv; cy *= inv; cz *= inv;
    const float Lx = box_old[4 * r], Ly = box_old[4 * r + 1], Lz = box_old[4 * r + 2];
    const float wx = cx - floorf(cx / Lx) * Lx, wy = cy - floorf(cy / Ly) * Ly, wz = cz - floorf(cz / Lz) * Lz;
    const float dx = wx * (scale - 1.f) - (cx - wx), dy = wy * (scale - 1.f) - (cy - wy), dz = wz * (scale - 1.f) - (cz - wz);
    for (int k = 0; k < n; ++k) { float4 p = P[a0 + k]; p.x += dx; p.y += dy; p.z += dz; P[a0 + k] = p; }
}

__global__ void baro_decide_kernel(int R, int r_begin, uint64_t seed, long long attempt, int n_mol, const double* __restrict__ U_old,
                                   const double* __restrict__ U_new, const int64_t* __restrict__ labels,
                                   const double* __restrict__ beta, const double* __restrict__ pressure,
                                   const double* __restrict__ econst, double econst_vref,
                                   float* __restrict__ box, const float* __restrict__ box_old, double* __restrict__ st,
                                   int* __restrict__ accepted, const unsigned int* __restrict__ noise_id,
                                   float min_edge, unsigned int* __restrict__ err)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double* S = st + (size_t)r * 8;
    const int k = (int)labels[r_begin + r];
    const double kT = 1.0 / beta[k];
    // + the current state's long-range constant ~ 1/V (alchemical sterics correction), which d_potential does not carry
    const double dlr = (econst_vref > 0.0) ? econst[k] * econst_vref * (1.0 / S[6] - 1.0 / S[7]) : 0.0;
    const double w = U_new[r] - U_old[r] + dlr + pressure[k] * S[5] - (double)n_mol * kT * log(S[6] / S[7]);
    const philox4 q = remd_philox(seed, REMD_STREAM_BAROSTAT, 1u, noise_id ? noise_id[r] : (uint32_t)(r_begin + r), (uint64_t)attempt);
    bool reject = !(w <= 0.0) && !(remd_u53(q.w[2], q.w[3]) <= exp(-w / kT));           // NaN energies reject
    // a trial box with an edge below twice the longer cutoff (the Coulomb range of the Ewald split may exceed the NonbondedForce
    // cutoff) was evaluated with a broken minimum image: never accept it, and say so -- OpenMM raises "The periodic box size has
    // decreased to less than twice the nonbonded cutoff" here (sticky device flag 6: api.hip turns it into the error)
    if (fminf(box[4 * r], fminf(box[4 * r + 1], box[4 * r + 2])) < min_edge) { reject = true; atomicCAS(err, 0u, 6u); }
    accepted[r] = reject ? 0 : 1;
    if (reject) { box[4 * r] = box_old[4 * r]; box[4 * r + 1] = box_old[4 * r + 1]; box[4 * r + 2] = box_old[4 * r + 2]; }
    else { S[2] += 1.0; S[4] += 1.0; }
    S[1] += 1.0; S[3] += 1.0;
    if (S[1] >= 10.0) {
        const double V = (double)box[4 * r] * (double)box[4 * r + 1] * (double)box[4 * r + 2];
        if (S[2] < 0.25 * S[1]) { S[0] /= 1.1; S[1] = 0.0; S[2] = 0.0; }
        else if (S[2] > 0.75 * S[1]) { S[0] = fmin(S[0] * 1.1, V * 0.3); S[1] = 0.0; S[2] = 0.0; }
    }
}

__global__ __launch_bounds__(256)
void baro_restore_kernel(int N, int Npad, const int* __restrict__ accepted, float4* __restrict__ pos, const float4* __restrict__ x0,
                         long long* __restrict__ force, const long long* __restrict__ f0, double* __restrict__ potential,
                         const double* __restrict__ U0)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (accepted[r]) return;
    if (i == 0) potential[r] = U0[r];
    if (i >= N) return;
    const size_t o = (size_t)r * Npad, of = (size_t)r * 3 * Npad;
    pos[o + i] = x0[o + i];
    force[of + i] = f0[of + i]; force[of + Npad + i] = f0[of + Npad + i]; force[of + 2 * Npad + i] = f0[of + 2 * Npad + i];
}

// ---------------------------------------------------------------------------------------------------
// Per-axis barostats (include/remd_hip_barostat.h): OpenMM's MonteCarloAnisotropicBarostatImpl and MonteCarloMembraneBarostatImpl,
// restated.  Every attempt draws ONE axis among the allowed ones (anisotropic: the scaled axes; membrane: x, y under XYAnisotropic,
// z under ZFree), changes the volume by dV = volumeScale[axis] * 2 (u - 1/2) and turns f = V'/V into the scale factors of the three
// edges: s[axis] = f, except that a membrane with an isotropic xy plane scales x and y by sqrt(f) together, and that under
// ConstantVolume z takes 1 / (sx sy) so that V' = V.  Molecules move as in baro_scale_kernel, component by component;
//   w = U' - U + p dV - gamma dA - N_mol kT ln(V'/V),   dA = Lx sx Ly sy - Lx Ly   (gamma = 0 for the anisotropic kind),
// the same Metropolis test and min-edge refusal as the isotropic move, and the same step adaptation kept per axis.
// Per-replica state, REMD_BARO_AXIS_STRIDE doubles: volumeScale[3], window attempted[3], window accepted[3], total attempted[3],
// total accepted[3], then the attempt under way: axis, dV, V', V, dA, s[3].
enum { BA_SCALE = 0, BA_WIN_ATT = 3, BA_WIN_ACC = 6, BA_TOT_ATT = 9, BA_TOT_ACC = 12, BA_AXIS = 15, BA_DV = 16, BA_NEWV = 17, BA_OLDV = 18,
       BA_DA = 19, BA_S = 20 };

__global__ void baro_axis_draw_kernel(int R, int r_begin, uint64_t seed, long long attempt, int kind, int axes, int zmode,
                                      float* __restrict__ box, float* __restrict__ box_old, double* __restrict__ st,
                                      const unsigned int* __restrict__ noise_id)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double* S = st + (size_t)r * REMD_BARO_AXIS_STRIDE;
    const double L[3] = { box[4 * r], box[4 * r + 1], box[4 * r + 2] };
    const double V = L[0] * L[1] * L[2];
    if (S[BA_SCALE] <= 0.0) { S[BA_SCALE] = 0.01 * V; S[BA_SCALE + 1] = 0.01 * V; S[BA_SCALE + 2] = 0.01 * V; }
    const bool membrane = kind == REMD_BAROSTAT_MEMBRANE;
    // the allowed axes, ascending, packed two bits each (no indexed private array)
    unsigned packed = 0; int n_allowed = 0;
    for (int a = 0; a < 3; ++a) {
        const bool on = membrane ? (a == 0 || (a == 1 && axes == REMD_BAROSTAT_XY_ANISOTROPIC) || (a == 2 && zmode == REMD_BAROSTAT_Z_FREE))
                                 : ((axes >> a) & 1);
        if (on) { packed |= (unsigned)a << (2 * n_allowed); ++n_allowed; }
    }
    const philox4 w = remd_philox(seed, REMD_STREAM_BAROSTAT, 0u, noise_id ? noise_id[r] : (uint32_t)(r_begin + r), (uint64_t)attempt);
    const int axis = (int)((packed >> (2 * remd_mulhi32(w.w[0], (uint32_t)n_allowed))) & 3u);
    const double vs = axis == 0 ? S[BA_SCALE] : (axis == 1 ? S[BA_SCALE + 1] : S[BA_SCALE + 2]);
    double dV = vs * 2.0 * (remd_u53(w.w[2], w.w[3]) - 0.5);
    double newV = V + dV;
    const double f = newV / V;
    double sx = 1.0, sy = 1.0, sz = 1.0;
    if (membrane && axis < 2 && axes == REMD_BAROSTAT_XY_ISOTROPIC) sx = sy = sqrt(f);
    else if (axis == 0) sx = f;
    else if (axis == 1) sy = f;
    else sz = f;
    if (membrane && zmode == REMD_BAROSTAT_CONSTANT_VOLUME) { sz = 1.0 / (sx * sy); newV = V; dV = 0.0; }
    S[BA_AXIS] = (double)axis; S[BA_DV] = dV; S[BA_NEWV] = newV; S[BA_OLDV] = V;
    S[BA_DA] = L[0] * sx * L[1] * sy - L[0] * L[1];
    S[BA_S] = sx; S[BA_S + 1] = sy; S[BA_S + 2] = sz;
    box_old[4 * r] = box[4 * r]; box_old[4 * r + 1] = box[4 * r + 1]; box_old[4 * r + 2] = box[4 * r + 2];
    box[4 * r] = (float)(L[0] * sx); box[4 * r + 1] = (float)(L[1] * sy); box[4 * r + 2] = (float)(L[2] * sz);
}

// one thread per molecule, as baro_scale_kernel, with a scale factor per component
__global__ __launch_bounds__(256)
void baro_axis_scale_kernel(int n_mol, const int* __restrict__ first, const int* __restrict__ size, int Npad,
                            float4* __restrict__ pos, const float* __restrict__ box_old, const double* __restrict__ st)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (g >= n_mol) return;
    const double* S = st + (size_t)r * REMD_BARO_AXIS_STRIDE;
    const float sx = (float)S[BA_S], sy = (float)S[BA_S + 1], sz = (float)S[BA_S + 2];
    float4* P = pos + (size_t)r * Npad;
    const int a0 = first[g], n = size[g];
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int k = 0; k < n; ++k) { const float4 p = P[a0 + k]; cx += p.x; cy += p.y; cz += p.z; }
    const float inv = 1.f / (float)n;
    cx *= inv; cy *= inv; cz *= inv;
    const float Lx = box_old[4 * r], Ly = box_old[4 * r + 1], Lz = box_old[4 * r + 2];
    const float wx = cx - floorf(cx / Lx) * Lx, wy = cy - floorf(cy / Ly) * Ly, wz = cz - floorf(cz / Lz) * Lz;
    const float dx = wx * (sx - 1.f) - (cx - wx), dy = wy * (sy - 1.f) - (cy - wy), dz = wz * (sz - 1.f) - (cz - wz);
    for (int k = 0; k < n; ++k) { float4 p = P[a0 + k]; p.x += dx; p.y += dy; p.z += dz; P[a0 + k] = p; }
}

__global__ void baro_axis_decide_kernel(int R, int r_begin, uint64_t seed, long long attempt, int n_mol, const double* __restrict__ U_old,
                                        const double* __restrict__ U_new, const int64_t* __restrict__ labels,
                                        const double* __restrict__ beta, const double* __restrict__ pressure,
                                        const double* __restrict__ tension /*[K] or null*/,
                                        const double* __restrict__ econst, double econst_vref,
                                        float* __restrict__ box, const float* __restrict__ box_old, double* __restrict__ st,
                                        int* __restrict__ accepted, const unsigned int* __restrict__ noise_id,
                                        float min_edge, unsigned int* __restrict__ err)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double* S = st + (size_t)r * REMD_BARO_AXIS_STRIDE;
    const int k = (int)labels[r_begin + r];
    const double kT = 1.0 / beta[k];
    const double newV = S[BA_NEWV], oldV = S[BA_OLDV];
    const double dlr = (econst_vref > 0.0) ? econst[k] * econst_vref * (1.0 / newV - 1.0 / oldV) : 0.0;
    const double gamma = tension ? tension[k] : 0.0;
    const double w = U_new[r] - U_old[r] + dlr + pressure[k] * S[BA_DV] - gamma * S[BA_DA] - (double)n_mol * kT * log(newV / oldV);
    const philox4 q = remd_philox(seed, REMD_STREAM_BAROSTAT, 1u, noise_id ? noise_id[r] : (uint32_t)(r_begin + r), (uint64_t)attempt);
    bool reject = !(w <= 0.0) && !(remd_u53(q.w[2], q.w[3]) <= exp(-w / kT));           // NaN energies reject
    // (the min-edge refusal of baro_decide_kernel: sticky device flag 6)
    if (fminf(box[4 * r], fminf(box[4 * r + 1], box[4 * r + 2])) < min_edge) { reject = true; atomicCAS(err, 0u, 6u); }
    accepted[r] = reject ? 0 : 1;
    if (reject) { box[4 * r] = box_old[4 * r]; box[4 * r + 1] = box_old[4 * r + 1]; box[4 * r + 2] = box_old[4 * r + 2]; }
    const int axis = (int)S[BA_AXIS];
    // the drawn axis' slots, by pointer arithmetic on the replica's row (axis is 0, 1 or 2)
    double* A = S + axis;
    if (!reject) { A[BA_WIN_ACC] += 1.0; A[BA_TOT_ACC] += 1.0; }
    A[BA_WIN_ATT] += 1.0; A[BA_TOT_ATT] += 1.0;
    if (A[BA_WIN_ATT] >= 10.0) {
        const double V = (double)box[4 * r] * (double)box[4 * r + 1] * (double)box[4 * r + 2];
        if (A[BA_WIN_ACC] < 0.25 * A[BA_WIN_ATT]) { A[BA_SCALE] /= 1.1; A[BA_WIN_ATT] = 0.0; A[BA_WIN_ACC] = 0.0; }
        else if (A[BA_WIN_ACC] > 0.75 * A[BA_WIN_ATT]) { A[BA_SCALE] = fmin(A[BA_SCALE] * 1.1, V * 0.3); A[BA_WIN_ATT] = 0.0; A[BA_WIN_ACC] = 0.0; }
    }
}

// u_kl of a membrane handle: rows[r][l] -= beta_l gamma_l Lx_r Ly_r (states.py:1915-1916), behind the assembly of the rows
__global__ void tension_ukl_kernel(int R, int K, const double* __restrict__ beta, const double* __restrict__ tension,
                                   const float* __restrict__ box, double* __restrict__ ukl_rows)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * K) return;
    const int r = t / K, l = t % K;
    ukl_rows[t] -= beta[l] * tension[l] * ((double)box[4 * r] * (double)box[4 * r + 1]);
}

int remd_tension_ukl(remd_ctx* h, double* d_rows)
{
    const int n = h->R * h->K;
    hipLaunchKernelGGL(tension_ukl_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->R, h->K, h->d_beta, h->d_tension, h->d_box, d_rows);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

int remd_barostat_buffers(remd_ctx* h)
{
    const int R = h->R, Npad = h->Npad;
    if (!h->d_baro) {
        REMD_TRY(h->d_baro.alloc(h, 8 * (size_t)R)); REMD_CHECK(h, hipMemsetAsync(h->d_baro, 0, sizeof(double) * 8 * R, h->stream));
        REMD_TRY(h->d_box_old.alloc(h, 4 * R));
        REMD_TRY(h->d_baro_x0.alloc(h, (size_t)R * Npad));
        REMD_TRY(h->d_baro_f0.alloc(h, 3 * (size_t)R * Npad));
        REMD_TRY(h->d_baro_U0.alloc(h, R));
        REMD_TRY(h->d_baro_acc.alloc(h, R));
    }
    if (h->baro_kind && !h->d_baro_axis) {
        REMD_TRY(h->d_baro_axis.alloc(h, REMD_BARO_AXIS_STRIDE * (size_t)R));
        REMD_CHECK(h, hipMemsetAsync(h->d_baro_axis, 0, sizeof(double) * REMD_BARO_AXIS_STRIDE * R, h->stream));
    }
    return 0;
}

int remd_barostat_attempt(remd_ctx* h)
{
    const int* grp_first = nullptr; const int* grp_size = nullptr;
    int n_groups = remd_nb_molecules(h, &grp_first, &grp_size);
    if (n_groups <= 0) n_groups = remd_custom_molecules(h, &grp_first, &grp_size);     // (a System whose only pair force is a CustomNonbondedForce)
    if (n_groups <= 0) return remd_fail(h, -3, "barostat: the system has no molecule table (needs a NonbondedForce, or a CutoffPeriodic CustomNonbondedForce whose molecules are contiguous and joined by custom forces only)");
    const int R = h->R, Npad = h->Npad;
    int rc;
    if ((rc = remd_barostat_buffers(h))) return rc;
    h->force_zeroed = false;
    if ((rc = remd_compute_forces(h, true))) return rc;                         // U and forces of the current configuration
    REMD_CHECK(h, hipMemcpyAsync(h->d_baro_U0, h->d_potential, sizeof(double) * R, hipMemcpyDeviceToDevice, h->stream));
    REMD_CHECK(h, hipMemcpyAsync(h->d_baro_f0, h->d_force, sizeof(long long) * 3 * (size_t)R * Npad, hipMemcpyDeviceToDevice, h->stream));
    REMD_CHECK(h, hipMemcpyAsync(h->d_baro_x0, h->d_pos, sizeof(float4) * (size_t)R * Npad, hipMemcpyDeviceToDevice, h->stream));
    const long long attempt = h->baro_attempts++;
    const bool axis_mode = h->baro_kind != 0;                                   // include/remd_hip_barostat.h
    if (axis_mode) {
        hipLaunchKernelGGL(baro_axis_draw_kernel, dim3((R + 63) / 64), dim3(64), 0, h->stream, R, h->r_begin, h->seed, attempt, h->baro_kind,
                           h->baro_axes, h->baro_zmode, h->d_box, h->d_box_old, h->d_baro_axis, h->d_noise_id);
        hipLaunchKernelGGL(baro_axis_scale_kernel, dim3((n_groups + 255) / 256, R), dim3(256), 0, h->stream, n_groups, grp_first,
                           grp_size, Npad, h->d_pos, h->d_box_old, h->d_baro_axis);
    } else {
    hipLaunchKernelGGL(baro_draw_kernel, dim3((R + 63) / 64), dim3(64), 0, h->stream, R, h->r_begin, h->seed, attempt, h->d_box,
                       h->d_box_old, h->d_baro, h->d_noise_id);
    hipLaunchKernelGGL(baro_scale_kernel, dim3((n_groups + 255) / 256, R), dim3(256), 0, h->stream, n_groups, grp_first,
                       grp_size, Npad, h->d_pos, h->d_box_old, h->d_baro);
    }
    h->box_uniform = false;                  // (every replica draws its own volume)
    h->box_version++;
    h->force_zeroed = false;
    if ((rc = remd_compute_forces(h, true))) return rc;                         // U' and forces of the scaled configuration
    if (axis_mode)
        hipLaunchKernelGGL(baro_axis_decide_kernel, dim3((R + 63) / 64), dim3(64), 0, h->stream, R, h->r_begin, h->seed, attempt, n_groups,
                           h->d_baro_U0, h->d_potential, h->d_labels, h->d_beta, h->d_pressure,
                           h->baro_kind == REMD_BAROSTAT_MEMBRANE ? (const double*)h->d_tension : (const double*)nullptr, h->d_econst, h->econst_vref,
                           h->d_box, h->d_box_old, h->d_baro_axis, h->d_baro_acc, h->d_noise_id,
                           (float)(2.0 * std::max(std::max(h->cutoff, h->coulomb_cutoff), h->cst_cutoff)), h->d_sync + 2);
    else
    hipLaunchKernelGGL(baro_decide_kernel, dim3((R + 63) / 64), dim3(64), 0, h->stream, R, h->r_begin, h->seed, attempt, n_groups,
                       h->d_baro_U0, h->d_potential, h->d_labels, h->d_beta, h->d_pressure, h->d_econst, h->econst_vref, h->d_box, h->d_box_old, h->d_baro,
                       h->d_baro_acc, h->d_noise_id, (float)(2.0 * std::max(std::max(h->cutoff, h->coulomb_cutoff), h->cst_cutoff)), h->d_sync + 2);
    hipLaunchKernelGGL(baro_restore_kernel, dim3((h->N + 255) / 256, R), dim3(256), 0, h->stream, h->N, Npad, h->d_baro_acc, h->d_pos,
                       h->d_baro_x0, h->d_force, h->d_baro_f0, h->d_potential, h->d_baro_U0);
    h->box_version++;
    h->forces_valid = true; h->force_zeroed = false;
    REMD_CHECK(h, hipGetLastError());
    return 0;
}


// ---- include/remd_hip_barostat.h ------------------------------------------------------------------
int remd_set_barostat_axes(remd_handle h, int K, const double* pressure, const double* surface_tension,
                           int kind, int xy_or_scale_mask, int zmode, int frequency)
{
    if (!h) return -1;
    if (!pressure || frequency <= 0) return remd_set_barostat(h, 0, nullptr, 0);
    if (kind == REMD_BAROSTAT_ANISOTROPIC) {
        if (xy_or_scale_mask < 1 || xy_or_scale_mask > 7) return remd_fail(h, -1, "remd_set_barostat_axes: the anisotropic barostat needs a scale mask of 1..7");
        surface_tension = nullptr; zmode = 0;
    } else if (kind == REMD_BAROSTAT_MEMBRANE) {
        if (xy_or_scale_mask != REMD_BAROSTAT_XY_ISOTROPIC && xy_or_scale_mask != REMD_BAROSTAT_XY_ANISOTROPIC)
            return remd_fail(h, -1, "remd_set_barostat_axes: unknown xy mode");
        if (zmode != REMD_BAROSTAT_Z_FREE && zmode != REMD_BAROSTAT_Z_FIXED && zmode != REMD_BAROSTAT_CONSTANT_VOLUME)
            return remd_fail(h, -1, "remd_set_barostat_axes: unknown z mode");
    } else return remd_fail(h, -1, "remd_set_barostat_axes: kind is REMD_BAROSTAT_ANISOTROPIC or REMD_BAROSTAT_MEMBRANE");
    std::vector<double> g(K > 0 ? K : 0, 0.0);
    if (surface_tension) for (int k = 0; k < K; ++k) {
        if (!(surface_tension[k] == surface_tension[k])) return remd_fail(h, -1, "remd_set_barostat_axes: NaN surface tension");
        g[k] = surface_tension[k];
    }
    const int kind0 = h->baro_kind;
    int rc = remd_set_barostat(h, K, pressure, frequency);          // pressures, frequency, K check (and back to the isotropic move)
    if (rc) return rc;
    hipSetDevice(h->device);
    if ((rc = h->d_tension.upload(h, g))) return rc;
    if (kind0 != kind || h->baro_axes != xy_or_scale_mask || h->baro_zmode != zmode || h->tension_host != g) h->config_version++;
    if ((kind0 != kind || h->baro_axes != xy_or_scale_mask || h->baro_zmode != zmode) && h->d_baro_axis) {
        REMD_CHECK(h, hipStreamSynchronize(h->stream));        // another move: its step sizes and counts start afresh
        h->d_baro_axis.reset();
    }
    h->baro_kind = kind; h->baro_axes = xy_or_scale_mask; h->baro_zmode = zmode; h->tension_host = g;
    return 0;
}

int remd_get_barostat_axis_stats(remd_handle h, double* volume_scale, int64_t* n_attempted, int64_t* n_accepted)
{
    if (!h || h->R <= 0) return remd_fail(h, -1, "remd_get_barostat_axis_stats: replicas not set");
    hipSetDevice(h->device);
    std::vector<double> st(REMD_BARO_AXIS_STRIDE * (size_t)h->R, 0.0);
    if (h->d_baro_axis) {
        REMD_CHECK(h, hipMemcpyAsync(st.data(), h->d_baro_axis, sizeof(double) * st.size(), hipMemcpyDeviceToHost, h->stream));
        REMD_CHECK(h, hipStreamSynchronize(h->stream));
    }
    for (int r = 0; r < h->R; ++r) for (int a = 0; a < 3; ++a) {
        const double* S = st.data() + (size_t)r * REMD_BARO_AXIS_STRIDE;
        if (volume_scale) volume_scale[3 * r + a] = S[BA_SCALE + a];
        if (n_attempted) n_attempted[3 * r + a] = (int64_t)S[BA_TOT_ATT + a];
        if (n_accepted) n_accepted[3 * r + a] = (int64_t)S[BA_TOT_ACC + a];
    }
    return 0;
}
