// Centroid-bond forces (include/remd_hip_custom.h, REMD_CUSTOM_CENTROID): OpenMM's CustomCentroidBondForce, a compound-bond expression
// whose particles are the weighted centroids of groups of atoms -- centre-of-mass distances, angles and dihedrals, Boresch restraints
// anchored on groups.  Three launches per force evaluation, behind one another on the stream of the listed terms, issued only for a
// handle that holds such a force:
//
//  1. centroids, grid (groups of all centroid forces, R), ONE wavefront per group: c = x_first + sum_i w_i img(x_i - x_first) in f64
//     (centroid_sum.h, the code and the convention of restraints.hip), each lane a strided share of the group's atoms, then a
//     xor-shuffle tree -> C[r][group][3].  One wavefront because a group is tens to a few hundred atoms: 64 lanes take a cucurbituril
//     in two trips, and a workgroup of one wavefront needs neither LDS nor a barrier.
//  2. bonds: the layout of custom_compound.hip (one thread per bond, one wavefront per workgroup, blockIdx.y the replica; 44 KiB of
//     static LDS), the wavefronts behind the compound-bond forces' in the padded term space, so the energy and u_kl reductions of
//     custom_terms.hip pick them up in descriptor order.  The lane's X[q] comes from C instead of from the positions, and the result of
//     the pass seeded at p, dE/d(centroid p), goes in f64 to G[r][slot][p][3] instead of to an atom.
//  3. spread, grid (groups, R), one wavefront per group: every lane adds, in table order, the G entries of each (bond, position) that
//     names the group (the host lists them per group, remd_set_custom_terms) -- the same sum in every lane, no exchange -- and gives
//     its strided share of the group's atoms -w_i g through add_force, rounded to f32 only there.  A group that no bond names leaves
//     after reading two offsets.
//
// Nothing here adds floating-point numbers atomically: C, G and the forces (fixed-point accumulators) depend on the input alone.
// The u_kl kernel is custom_compound.hip's reading C, behind a centroid launch of its own on the main stream.
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"
#include "centroid_sum.h"

namespace {

constexpr int CEN_P = REMD_CUSTOM_MAX_PARTICLES;        // the stride of a bond's slots in G

// grid (n_groups, R), 64 threads
__global__ __launch_bounds__(64)
void custom_centroid_sum_kernel(int n_groups, const int* __restrict__ grp_off, const int* __restrict__ grp_atoms,
                                const double* __restrict__ grp_w, const int* __restrict__ grp_periodic, int Npad,
                                const float4* __restrict__ pos, const float* __restrict__ box, double* __restrict__ C /*[R][n_groups][3]*/)
{
    const int g = blockIdx.x, r = blockIdx.y;
    const int b = grp_off[g], n = grp_off[g + 1] - b;
    const double3 c = centroid<64>(pos + (size_t)r * Npad, grp_atoms, grp_w, b, n, grp_periodic[g] != 0, box[4 * r], box[4 * r + 1],
                                   box[4 * r + 2], nullptr);
    if (threadIdx.x == 0) {
        double* o = C + ((size_t)r * n_groups + g) * 3;
        o[0] = c.x; o[1] = c.y; o[2] = c.z;
    }
}

// the centroids of the lane's groups -> X; the bond's slot s in the padded term space
__device__ __forceinline__ void cen_load(const cst_force& f, const int* __restrict__ atoms, int total_pad, int s, const double* __restrict__ Cr,
                                         cst_pos* X, int lane)
{
    for (int q = 0; q < f.n_particles; ++q) {
        const double* c = Cr + (size_t)atoms[(size_t)q * total_pad + s] * 3;
        X[q][0][lane] = c[0]; X[q][1][lane] = c[1]; X[q][2][lane] = c[2];
    }
}

// grid (wavefronts of the centroid forces, R), 64 threads; w0: the first of them in the padded term space of `waves` wavefronts
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_centroid_bonds_kernel(int total_pad, int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                                  const int* __restrict__ atoms, const double* __restrict__ par, const int2* __restrict__ prog,
                                  const double* __restrict__ consts, const double* __restrict__ glob /*[K][ng]*/, int ng,
                                  const int64_t* __restrict__ labels, int r_begin, int n_groups, const double* __restrict__ C,
                                  const float* __restrict__ box, double* __restrict__ G /*[R][(waves - w0) 64][CEN_P][3]*/,
                                  double* __restrict__ Ewave /*[R][waves]*/)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[REMD_CUSTOM_MAX_PARTICLES];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const bool pbc = f.periodic != 0;                       // (box lengths 0: cst_image leaves a difference as it is)
    const double Lx = pbc ? box[4 * r] : 0.0, Ly = pbc ? box[4 * r + 1] : 0.0, Lz = pbc ? box[4 * r + 2] : 0.0;
    const double* g = glob + (size_t)labels[r_begin + r] * ng;
    cen_load(f, atoms, total_pad, s, C + (size_t)r * n_groups * 3, X, lane);
    const bool active = t < f.n_terms;
    double* Gs = G + (((size_t)r * (waves - w0) + blockIdx.x) * 64 + lane) * CEN_P * 3;
    double e0 = 0.0;
    for (int p = 0; p < f.n_particles; ++p) {
        const cx e = cst_eval<true>(f, prog, consts, par, t, g, 0.0, 0.0, 0.0, Lx, Ly, Lz, S, lane, X, p);
        if (p == 0) e0 = e.v;
        if (active) { Gs[3 * p] = e.a; Gs[3 * p + 1] = e.b; Gs[3 * p + 2] = e.c; }
    }
    if (ENERGY) {
        const double ew = cst_wave_sum(active ? e0 : 0.0);
        if (lane == 0) Ewave[(size_t)r * waves + w] = ew;
    }
}

// grid (n_groups, R), 64 threads
__global__ __launch_bounds__(64)
void custom_centroid_spread_kernel(int n_groups, const int* __restrict__ grp_off, const int* __restrict__ grp_atoms,
                                   const double* __restrict__ grp_w, const int* __restrict__ ref_off, const int* __restrict__ refs,
                                   int n_slots, const double* __restrict__ G, int Npad, long long* __restrict__ force)
{
    const int g = blockIdx.x, r = blockIdx.y;
    const int k0 = ref_off[g], k1 = ref_off[g + 1];
    if (k0 == k1) return;
    const double* Gr = G + (size_t)r * n_slots * CEN_P * 3;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (int k = k0; k < k1; ++k) {
        const double* o = Gr + (size_t)refs[k] * 3;
        gx += o[0]; gy += o[1]; gz += o[2];
    }
    long long* Fr = force + (size_t)r * 3 * Npad;
    const int b = grp_off[g], n = grp_off[g + 1] - b;
    for (int k = threadIdx.x; k < n; k += 64) {
        const double wk = grp_w[b + k];
        add_force(Fr, Npad, grp_atoms[b + k], (float)(-wk * gx), (float)(-wk * gy), (float)(-wk * gz));
    }
}

// u_kl partials, grid (wavefronts of the centroid forces, R): D[r][l][w] = sum over the wavefront's bonds of e(g_l) - e(g_own), the
// difference formed per bond (custom_compound_ukl_kernel over the centroids)
__global__ __launch_bounds__(64)
void custom_centroid_ukl_kernel(int total_pad, int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                                const int* __restrict__ atoms, const double* __restrict__ par, const int2* __restrict__ prog,
                                const double* __restrict__ consts, const double* __restrict__ glob, int ng, int K,
                                const int64_t* __restrict__ labels, int r_begin, int n_groups, const double* __restrict__ C,
                                const float* __restrict__ box, double* __restrict__ D)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[REMD_CUSTOM_MAX_PARTICLES];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const bool pbc = f.periodic != 0;
    const double Lx = pbc ? box[4 * r] : 0.0, Ly = pbc ? box[4 * r + 1] : 0.0, Lz = pbc ? box[4 * r + 2] : 0.0;
    const double* g_own = glob + (size_t)labels[r_begin + r] * ng;
    cen_load(f, atoms, total_pad, s, C + (size_t)r * n_groups * 3, X, lane);
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

// energy parameter derivatives, same grid: custom_compound_dpar_kernel over the centroids
// STATES: under the globals of every state l in turn, D[r][l][d][w], behind the one load of the particles
template <bool STATES>
__global__ __launch_bounds__(64)
void custom_centroid_dpar_kernel(int total_pad, int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                                 const int* __restrict__ atoms, const double* __restrict__ par, const int2* __restrict__ prog,
                                 const double* __restrict__ consts, const double* __restrict__ glob, int ng, int nd,
                                 const int* __restrict__ dcols, const unsigned* __restrict__ dmask, const int64_t* __restrict__ labels,
                                 int r_begin, int n_groups, const double* __restrict__ C, const float* __restrict__ box, double* __restrict__ D, int K)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ cst_pos X[REMD_CUSTOM_MAX_PARTICLES];
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const unsigned mask = dmask[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const bool pbc = f.periodic != 0;
    const double Lx = pbc ? box[4 * r] : 0.0, Ly = pbc ? box[4 * r + 1] : 0.0, Lz = pbc ? box[4 * r + 2] : 0.0;
    cen_load(f, atoms, total_pad, s, C + (size_t)r * n_groups * 3, X, lane);
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

void launch_centroids(remd_ctx* h, cst_tables& t, hipStream_t st)
{
    remd_prof_scope ps(h, "custom_centroid_sum", st);
    hipLaunchKernelGGL(custom_centroid_sum_kernel, dim3(t.n_groups, h->R), dim3(64), 0, st, t.n_groups, t.d_grp_off, t.d_grp_atoms, t.d_grp_w,
                       t.d_grp_periodic, h->Npad, h->d_pos, h->d_box, t.d_C);
}

}  // namespace

// (the caller, remd_custom_forces, has sized d_C and d_G: ensure_buffers of custom_terms.hip)
void remd_custom_centroid_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_CENTROID);
    launch_centroids(h, t, st);
    {
        remd_prof_scope ps(h, "custom_centroid_bonds", st);
        if (with_energy)
            hipLaunchKernelGGL(custom_centroid_bonds_kernel<true>, dim3(t.end(CST_CENTROID) - w0, h->R), dim3(64), 0, st, t.total_pad, w0, waves, t.d_F,
                               t.d_wave_force, t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, t.n_groups,
                               t.d_C, h->d_box, t.d_G, t.d_Ewave);
        else
            hipLaunchKernelGGL(custom_centroid_bonds_kernel<false>, dim3(t.end(CST_CENTROID) - w0, h->R), dim3(64), 0, st, t.total_pad, w0, waves, t.d_F,
                               t.d_wave_force, t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, t.n_groups,
                               t.d_C, h->d_box, t.d_G, t.d_Ewave);
    }
    remd_prof_scope ps(h, "custom_centroid_spread", st);
    hipLaunchKernelGGL(custom_centroid_spread_kernel, dim3(t.n_groups, h->R), dim3(64), 0, st, t.n_groups, t.d_grp_off, t.d_grp_atoms, t.d_grp_w,
                       t.d_ref_off, t.d_refs, (waves - w0) * 64, t.d_G, h->Npad, h->d_force);
}

void remd_custom_centroid_ukl(remd_ctx* h, cst_tables& t)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_CENTROID);
    launch_centroids(h, t, h->stream);
    hipLaunchKernelGGL(custom_centroid_ukl_kernel, dim3(t.end(CST_CENTROID) - w0, h->R), dim3(64), 0, h->stream, t.total_pad, w0, waves, t.d_F, t.d_wave_force,
                       t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->K, h->d_labels, h->r_begin, t.n_groups, t.d_C, h->d_box,
                       t.d_D);
}

// (the caller has sized d_C: ensure_buffers of custom_terms.hip)
void remd_custom_centroid_dpar(remd_ctx* h, cst_tables& t, bool states)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_CENTROID);
    launch_centroids(h, t, h->stream);
    const dim3 grid(t.end(CST_CENTROID) - w0, h->R);
    if (states)
        hipLaunchKernelGGL(custom_centroid_dpar_kernel<true>, grid, dim3(64), 0, h->stream, t.total_pad, w0, waves, t.d_F, t.d_wave_force,
                           t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, (int)t.dcols.size(), t.d_dcols, t.d_dmask, h->d_labels, h->r_begin,
                           t.n_groups, t.d_C, h->d_box, t.d_dDK, h->K);
    else
        hipLaunchKernelGGL(custom_centroid_dpar_kernel<false>, grid, dim3(64), 0, h->stream, t.total_pad, w0, waves, t.d_F, t.d_wave_force,
                           t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, (int)t.dcols.size(), t.d_dcols, t.d_dmask, h->d_labels, h->r_begin,
                           t.n_groups, t.d_C, h->d_box, t.d_dD, 1);
}
