// CMAP torsion forces (include/remd_hip_custom.h, REMD_CUSTOM_CMAP): OpenMM's CMAPTorsionForce, the energy of a pair of dihedrals read
// from one of the force's periodic maps -- the backbone phi / psi correction of CHARMM22/36 and Amber ff19SB.
//
// The layout is that of custom_terms.hip: one lane per torsion pair, a workgroup is ONE wavefront and holds terms of one force (padded
// to 64 with the last term repeated; a padding lane reads that term's tables and adds nothing), blockIdx.y is the replica.  The
// wavefronts lie behind those of the collective-variable forces, the last part of the padded term space, so the per-wavefront energies
// land in Ewave and custom_reduce_kernel adds them with the others in its fixed order.  The force has no globals: it writes no u_kl
// partials (remd_custom_ukl keeps its columns of D zero) and its energy reaches the rows through the replica's potential.
//
// No program, no stack, no LDS: the geometry is done once per term (cmap_math.h: both dihedrals with their gradients, the formulas of
// cst_particles_op), the term's map is picked by index -- map_index[slot] names one of the force's blocks in the constants, map_off its
// offset there -- and cst_table2d (table2d_patch.h) gives the patch's value and both partials.  Eight add_force calls hand
// -(dE/dphi) dphi/dx and -(dE/dpsi) dpsi/dx to the fixed-point accumulators (order-independent, bit-reproducible; rounded to f32 only
// there); a particle that both dihedrals name gets two.  remd_set_custom_terms has checked the atoms, the map indices and every
// block's header, and cst_table2d loads only inside a block whatever the angles are.
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"
#include "cmap_math.h"

namespace {

// grid (wavefronts of the CMAP forces, R), 64 threads; w0: the first of them in the padded term space of `waves` wavefronts
template <bool ENERGY>
__global__ __launch_bounds__(64)
void cmap_kernel(int total_pad, int w0, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force,
                 const int* __restrict__ atoms, const int* __restrict__ map_index /*[the CMAP forces' slots]*/, const int* __restrict__ map_off,
                 const double* __restrict__ consts, int Npad, const float4* __restrict__ pos, const float* __restrict__ box,
                 long long* __restrict__ force, double* __restrict__ Ewave /*[R][waves]*/)
{
    const int w = w0 + blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const float4* P = pos + (size_t)r * Npad;
    const bool pbc = f.periodic != 0;                       // (box lengths 0: cm_image leaves a difference as it is)
    const double Lx = pbc ? box[4 * r] : 0.0, Ly = pbc ? box[4 * r + 1] : 0.0, Lz = pbc ? box[4 * r + 2] : 0.0;
    int a[8]; float p[8][4];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        a[q] = atoms[(size_t)q * total_pad + s];
        const float4 x = P[a[q]];
        p[q][0] = x.x; p[q][1] = x.y; p[q][2] = x.z; p[q][3] = 0.0f;
    }
    const double* B = consts + map_off[f.map0 + map_index[s - w0 * 64]];
    cm3 G[8];
    const double v = cmap_term(B, p, Lx, Ly, Lz, G);
    const bool active = t < f.n_terms;
    if (active) {
        long long* Fr = force + (size_t)r * 3 * Npad;
#pragma unroll
        for (int q = 0; q < 8; ++q) add_force(Fr, Npad, a[q], (float)G[q].x, (float)G[q].y, (float)G[q].z);
    }
    if (ENERGY) {
        const double ew = cst_wave_sum(active ? v : 0.0);
        if (lane == 0) Ewave[(size_t)r * waves + w] = ew;
    }
}

}  // namespace

void remd_cmap_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st)
{
    const int waves = t.total_pad / 64, w0 = t.begin(CST_CMAP);
    if (with_energy)
        hipLaunchKernelGGL(cmap_kernel<true>, dim3(t.end(CST_CMAP) - w0, h->R), dim3(64), 0, st, t.total_pad, w0, waves, t.d_F, t.d_wave_force, t.d_atoms,
                           t.d_map_index, t.d_map_off, t.d_consts, h->Npad, h->d_pos, h->d_box, h->d_force, t.d_Ewave);
    else
        hipLaunchKernelGGL(cmap_kernel<false>, dim3(t.end(CST_CMAP) - w0, h->R), dim3(64), 0, st, t.total_pad, w0, waves, t.d_F, t.d_wave_force, t.d_atoms,
                           t.d_map_index, t.d_map_off, t.d_consts, h->Npad, h->d_pos, h->d_box, h->d_force, t.d_Ewave);
}
