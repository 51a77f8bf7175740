// Compound-bond forces (include/remd_hip_custom.h, REMD_CUSTOM_COMPOUND): OpenMM's CustomCompoundBondForce, an energy expression of the
// coordinates of P particles (1 ... REMD_CUSTOM_MAX_PARTICLES) and of the distances, angles and dihedrals between them -- Boresch
// restraints are one bond of six particles.
//
// The layout is that of custom_terms.hip: one thread per bond, a workgroup is ONE wavefront and holds bonds of one force (padded to
// 64 with the last bond repeated), blockIdx.y is the replica, and program, constants and globals are wave-uniform.  The wavefronts of
// the compound-bond forces lie behind those of the four one-variable kinds in the padded term space (and in front of the centroid
// forces', custom_centroid.hip), so the per-wavefront energy and
// u_kl partials land in the same arrays and custom_reduce_kernel / custom_ukl_reduce_kernel add them with the others.
//
// Derivatives by seeded passes: the energy depends on several geometric quantities of several particles, which one chain-rule factor
// cannot carry, and a slot with 3 P partials would not fit the LDS.  The machine stays a value and three partials (custom_machine.h)
// and the program runs once per particle p: in that pass x_p y_p z_p carry the unit partials, a distance / angle / dihedral pushes its
// gradient with respect to particle p, and the result's partials are dE/d(x_p, y_p, z_p), which go to that particle's atom through
// add_force (rounded to f32 only there).  The energy is the first pass's.  That is P program runs per force evaluation, for a
// handful of bonds: a latency-class launch.  The u_kl kernel runs unseeded, once per state whose globals differ from the replica's.
//
// A lane keeps its P particle positions in LDS as f64, [particle][component][lane] (12 KiB): the program addresses them by a
// wave-uniform index, which an array in registers would turn into scratch.  With the 32 KiB stack that is 44 KiB of static LDS.
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"

namespace {

// the lane's particles -> X; the bond's slot s in the padded term space
__device__ __forceinline__ void cmp_load(const cst_force& f, const int* __restrict__ atoms, int total_pad, int s, const float4* __restrict__ P,
                                         cst_pos* X, int lane)
{
    for (int q = 0; q < f.n_particles; ++q) {
        const float4 p = P[atoms[(size_t)q * total_pad + s]];
        X[q][0][lane] = (double)p.x; X[q][1][lane] = (double)p.y; X[q][2][lane] = (double)p.z;
    }
}

// grid (wavefronts of the compound-bond forces, R), 64 threads; w0: the first of them in the padded term space of `waves` wavefronts
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_compound_kernel(int total_pad, int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                            const int* __restrict__ atoms, const double* __restrict__ par, const int2* __restrict__ prog,
                            const double* __restrict__ consts, const double* __restrict__ glob /*[K][ng]*/, int ng,
                            const int64_t* __restrict__ labels, int r_begin, int Npad, const float4* __restrict__ pos,
                            const float* __restrict__ box, long long* __restrict__ force, double* __restrict__ Ewave /*[R][waves]*/)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[REMD_CUSTOM_MAX_PARTICLES];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const float4* P = pos + (size_t)r * Npad;
    const bool pbc = f.periodic != 0;                       // (box lengths 0: cst_image leaves a difference as it is)
    const double Lx = pbc ? box[4 * r] : 0.0, Ly = pbc ? box[4 * r + 1] : 0.0, Lz = pbc ? box[4 * r + 2] : 0.0;
    const double* g = glob + (size_t)labels[r_begin + r] * ng;
    cmp_load(f, atoms, total_pad, s, P, X, lane);
    const bool active = t < f.n_terms;
    long long* Fr = force + (size_t)r * 3 * Npad;
    double e0 = 0.0;
    for (int p = 0; p < f.n_particles; ++p) {
        const cx e = cst_eval<true>(f, prog, consts, par, t, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, p);
        if (p == 0) e0 = e.v;
        if (active) add_force(Fr, Npad, atoms[(size_t)p * total_pad + s], (float)-e.a, (float)-e.b, (float)-e.c);
    }
    if (ENERGY) {
        const double ew = cst_wave_sum(active ? e0 : 0.0);
        if (lane == 0) Ewave[(size_t)r * waves + w] = ew;
    }
}

// u_kl partials, grid (wavefronts of the compound-bond forces, R): D[r][l][w] = sum over the wavefront's bonds of e(g_l) - e(g_own), the
// difference formed per bond (as custom_ukl_kernel)
__global__ __launch_bounds__(64)
void custom_compound_ukl_kernel(int total_pad, int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                                const int* __restrict__ atoms, const double* __restrict__ par, const int2* __restrict__ prog,
                                const double* __restrict__ consts, const double* __restrict__ glob, int ng, int K,
                                const int64_t* __restrict__ labels, int r_begin, int Npad, const float4* __restrict__ pos,
                                const float* __restrict__ box, double* __restrict__ D)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[REMD_CUSTOM_MAX_PARTICLES];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const float4* P = pos + (size_t)r * Npad;
    const bool pbc = f.periodic != 0;
    const double Lx = pbc ? box[4 * r] : 0.0, Ly = pbc ? box[4 * r + 1] : 0.0, Lz = pbc ? box[4 * r + 2] : 0.0;
    const double* g_own = glob + (size_t)labels[r_begin + r] * ng;
    cmp_load(f, atoms, total_pad, s, P, X, lane);
    const bool active = t < f.n_terms;
    double e_own = 0.0;
    for (int l = -1; l < K; ++l) {
        const double* g = l < 0 ? g_own : glob + (size_t)l * ng;
        bool same = l >= 0;
        for (int i = 0; i < ng && same; ++i) same = g[i] == g_own[i];
        double d = 0.0;
        if (!same) {
            const double e = cst_eval<true>(f, prog, consts, par, t, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, -1).v;
            if (l < 0) e_own = e; else d = active ? e - e_own : 0.0;
        }
        if (l >= 0) {
            d = cst_wave_sum(d);
            if (lane == 0) D[((size_t)r * K + l) * waves + w] = d;
        }
    }
}

// energy parameter derivatives, same grid: D[r][d][w] = sum over the wavefront's bonds of dE/dglobal(dcols[d]) under the replica's own
// globals (custom_dpar_kernel of custom_terms.hip: the machine seeded at the column, no particle seeded)
// STATES: under the globals of every state l in turn, D[r][l][d][w], behind the one load of the particles
template <bool STATES>
__global__ __launch_bounds__(64)
void custom_compound_dpar_kernel(int total_pad, int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                                 const int* __restrict__ atoms, const double* __restrict__ par, const int2* __restrict__ prog,
                                 const double* __restrict__ consts, const double* __restrict__ glob, int ng, int nd,
                                 const int* __restrict__ dcols, const unsigned* __restrict__ dmask, const int64_t* __restrict__ labels,
                                 int r_begin, int Npad, const float4* __restrict__ pos, const float* __restrict__ box, double* __restrict__ D, int K)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[REMD_CUSTOM_MAX_PARTICLES];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const unsigned mask = dmask[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const float4* P = pos + (size_t)r * Npad;
    const bool pbc = f.periodic != 0;
    const double Lx = pbc ? box[4 * r] : 0.0, Ly = pbc ? box[4 * r + 1] : 0.0, Lz = pbc ? box[4 * r + 2] : 0.0;
    cmp_load(f, atoms, total_pad, s, P, X, lane);
    const bool active = t < f.n_terms;
    const int nl = STATES ? K : 1;
    for (int l = 0; l < nl; ++l) {
        const double* g = glob + (size_t)(STATES ? l : labels[r_begin + r]) * ng;
        for (int d = 0; d < nd; ++d) {
            double v = 0.0;
            if ((mask >> d) & 1u) {
                const cx e = cst_eval<true, true>(f, prog, consts, par, t, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, -1, dcols[d]);
                v = cst_wave_sum(active ? e.a : 0.0);
            }
            if (lane == 0) D[(((size_t)r * nl + l) * nd + d) * waves + w] = v;
        }
    }
}

}  // namespace

void remd_custom_compound_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_COMPOUND);
    if (with_energy)
        hipLaunchKernelGGL(custom_compound_kernel<true>, dim3(t.end(CST_COMPOUND) - w0, h->R), dim3(64), 0, st, t.total_pad, w0, waves, t.d_F, t.d_wave_force,
                           t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, h->Npad, h->d_pos, h->d_box,
                           h->d_force, t.d_Ewave);
    else
        hipLaunchKernelGGL(custom_compound_kernel<false>, dim3(t.end(CST_COMPOUND) - w0, h->R), dim3(64), 0, st, t.total_pad, w0, waves, t.d_F, t.d_wave_force,
                           t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, h->Npad, h->d_pos, h->d_box,
                           h->d_force, t.d_Ewave);
}

void remd_custom_compound_ukl(remd_ctx* h, cst_tables& t)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_COMPOUND);
    hipLaunchKernelGGL(custom_compound_ukl_kernel, dim3(t.end(CST_COMPOUND) - w0, h->R), dim3(64), 0, h->stream, t.total_pad, w0, waves, t.d_F, t.d_wave_force,
                       t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->K, h->d_labels, h->r_begin, h->Npad, h->d_pos, h->d_box,
                       t.d_D);
}

void remd_custom_compound_dpar(remd_ctx* h, cst_tables& t, bool states)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_COMPOUND);
    const dim3 grid(t.end(CST_COMPOUND) - w0, h->R);
    if (states)
        hipLaunchKernelGGL(custom_compound_dpar_kernel<true>, grid, dim3(64), 0, h->stream, t.total_pad, w0, waves, t.d_F, t.d_wave_force,
                           t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, (int)t.dcols.size(), t.d_dcols, t.d_dmask, h->d_labels, h->r_begin,
                           h->Npad, h->d_pos, h->d_box, t.d_dDK, h->K);
    else
        hipLaunchKernelGGL(custom_compound_dpar_kernel<false>, grid, dim3(64), 0, h->stream, t.total_pad, w0, waves, t.d_F, t.d_wave_force,
                           t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, (int)t.dcols.size(), t.d_dcols, t.d_dmask, h->d_labels, h->r_begin,
                           h->Npad, h->d_pos, h->d_box, t.d_dD, 1);
}
