// Custom bond, angle, torsion and external forces (include/remd_hip_custom.h): OpenMM's CustomBondForce / CustomAngleForce /
// CustomTorsionForce / CustomExternalForce with an energy expression the host compiled into a postfix program
// (openmmtools_amd/custom_expr.py).
//
// One thread per term, every term of every custom force of a replica in one launch (blockIdx.y = replica).  A workgroup is ONE
// wavefront and holds terms of one force only (each force's terms are padded to whole wavefronts; a padding lane repeats the
// force's last term and adds nothing), so the program counter, the opcode dispatch and the reads of the program, the constants and
// the global parameters are wave-uniform: only the operands differ per lane.  The machine is forward-mode: every stack slot holds a
// value and its three partial derivatives with respect to the force's variables (r or theta use the first, x y z all three), so the
// result's partials are dE/dr, dE/dtheta or the gradient, and the term's atoms get -dE/dvar times the variable's gradient through
// the fixed-point accumulators (order-independent sums).  The stack lives in LDS, [slot][component][lane]: an array indexed by the
// stack pointer in registers would go to scratch memory.
//
// Arithmetic: f64 throughout -- geometry, the machine, the gradients; only the force handed to add_force is rounded to f32.  Where
// f64 is needed: per-term parameters cancel against coordinates (x - x0 of a position restraint: x0 rounded to f32 alone is 1e-5 of
// a 0.01 nm displacement), theta near 0 and pi, and the u_kl differences E(g_l) - E(g_own), which are formed per term before they
// are summed.  An interpreter cannot tell a subtraction that cancels from one that does not, so the whole machine is f64.  Measured
// (profiles/custom_terms_cost.txt): 8.8 us per launch at 1 wavefront x 8 replicas, 15.2 us at 16 wavefronts x 8 replicas (924 terms of
// the built-in bonded formulas, which the built-in kernel does in 2.3 us); what share of that is f64 arithmetic and what the
// interpreter itself (LDS stack, dispatch) has not been separated -- an fp32 machine with f64 differences is the next experiment.
//
// Energies: a wavefront sums its terms by a xor-shuffle tree, the partial goes to [R][wavefronts], and a second one-wavefront launch
// per replica adds each force's partials in a fixed order -> [R][n_forces] and the replica's energy partial (the restraints' slot,
// the last one: added behind the restraint kernel on the same stream).  No atomics touch an energy.
//
// The machine itself (cst_eval) lives in custom_machine.h: custom_compound.hip runs the same one for CustomCompoundBondForce, whose
// wavefronts follow the ones of this file's four kinds in the padded term space and share the energy and u_kl reductions below, and
// custom_centroid.hip runs it for CustomCentroidBondForce, whose wavefronts come last; custom_nonbonded.hip runs it for
// CustomNonbondedForce, one wavefront per tile of 64 x 64 atoms, between those two; custom_cv.hip runs it for CustomCVForce, one
// wavefront per force behind the centroid forces', its variables the RMSDs a launch of its own computed.  cmap.hip (CMAPTorsionForce)
// runs no program: it shares the term space, the tables and the energy reduction only.  custom_hbond.hip runs the machine for
// CustomHbondForce, one wavefront per tile of 64 donors x 64 acceptors, and custom_manyparticle.hip for CustomManyParticleForce, one
// wavefront per central particle behind a neighbour search of its own; each new part comes last, so that no other kind's slot depends on it.
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"

void remd_table_deleter::operator()(cst_tables* t) const { delete t; }

namespace {

struct cst_geom {
    int a0, a1, a2, a3;
    double x0, x1, x2;                // the force's variables: r / theta / x, then y, z of an external force
    double3 g0, g1, g2, g3;           // gradient of the ONE variable of a bond / angle / torsion with respect to each atom
};

// the variables of slot s of force f: the formulas of listed_terms.h (listed_bond / listed_angle / listed_torsion) in f64
__device__ __forceinline__ void cst_geometry(const cst_force& f, const int* __restrict__ atoms, int total_pad, int s,
                                             const float4* __restrict__ P, double Lx, double Ly, double Lz, cst_geom& o)
{
    const bool pbc = f.periodic != 0;
    const double3 zero = d3(0.0, 0.0, 0.0);
    o.a0 = atoms[s]; o.a1 = o.a2 = o.a3 = 0;
    o.x0 = o.x1 = o.x2 = 0.0;
    o.g0 = o.g1 = o.g2 = o.g3 = zero;
    if (f.kind == REMD_CUSTOM_EXTERNAL) {
        const float4 p = P[o.a0];
        o.x0 = (double)p.x; o.x1 = (double)p.y; o.x2 = (double)p.z;
    } else if (f.kind == REMD_CUSTOM_BOND) {
        o.a1 = atoms[total_pad + s];
        const double3 d = d3img(d3sub(P[o.a1], P[o.a0]), pbc, Lx, Ly, Lz);
        const double r = sqrt(d3dot(d, d)), ir = r > 0.0 ? 1.0 / r : 0.0;
        o.x0 = r;
        o.g1 = d3scl(d, ir); o.g0 = d3scl(d, -ir);
    } else if (f.kind == REMD_CUSTOM_ANGLE) {
        o.a1 = atoms[total_pad + s]; o.a2 = atoms[2 * total_pad + s];
        const double3 v0 = d3img(d3sub(P[o.a0], P[o.a1]), pbc, Lx, Ly, Lz), v1 = d3img(d3sub(P[o.a2], P[o.a1]), pbc, Lx, Ly, Lz);
        const double3 cp = d3crs(v0, v1);
        const double rp = fmax(sqrt(d3dot(cp, cp)), 1e-6);
        const double r20 = d3dot(v0, v0), r21 = d3dot(v1, v1);
        const double cosine = fmin(fmax(d3dot(v0, v1) / sqrt(r20 * r21), -1.0), 1.0);
        o.x0 = acos(cosine);
        o.g0 = d3scl(d3crs(v0, cp), 1.0 / (r20 * rp));
        o.g2 = d3scl(d3crs(cp, v1), 1.0 / (r21 * rp));
        o.g1 = d3scl(d3add(o.g0, o.g2), -1.0);
    } else {
        o.a1 = atoms[total_pad + s]; o.a2 = atoms[2 * total_pad + s]; o.a3 = atoms[3 * total_pad + s];
        const double3 b1 = d3img(d3sub(P[o.a1], P[o.a0]), pbc, Lx, Ly, Lz), b2 = d3img(d3sub(P[o.a2], P[o.a1]), pbc, Lx, Ly, Lz);
        const double3 b3 = d3img(d3sub(P[o.a3], P[o.a2]), pbc, Lx, Ly, Lz);
        const double3 m = d3crs(b1, b2), nn = d3crs(b2, b3);
        const double m2 = fmax(d3dot(m, m), 1e-24), n2 = fmax(d3dot(nn, nn), 1e-24);
        const double lb2 = sqrt(d3dot(b2, b2));
        o.x0 = atan2(lb2 * d3dot(b1, nn), d3dot(m, nn));
        o.g0 = d3scl(m, -lb2 / m2);
        o.g3 = d3scl(nn, lb2 / n2);
        const double s12 = d3dot(b1, b2) / (lb2 * lb2), s32 = d3dot(b3, b2) / (lb2 * lb2);
        o.g1 = d3add(d3scl(o.g0, -(1.0 + s12)), d3scl(o.g3, s32));
        o.g2 = d3add(d3scl(o.g3, -(1.0 + s32)), d3scl(o.g0, s12));
    }
}

// grid (wavefronts of the four kinds' part of the padded term space, R), 64 threads; `waves` counts those of the whole space
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_terms_kernel(int total_pad, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ atoms,
                         const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                         const double* __restrict__ glob /*[K][ng]*/, int ng, const int64_t* __restrict__ labels, int r_begin, int Npad,
                         const float4* __restrict__ pos, const float* __restrict__ box, long long* __restrict__ force,
                         double* __restrict__ Ewave /*[R][waves]*/)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    const int w = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const float4* P = pos + (size_t)r * Npad;
    const double Lx = box[4 * r], Ly = box[4 * r + 1], Lz = box[4 * r + 2];
    const double* g = glob + (size_t)labels[r_begin + r] * ng;
    cst_geom o;
    cst_geometry(f, atoms, total_pad, s, P, Lx, Ly, Lz, o);
    const cx e = cst_eval<false>(f, prog, consts, par, t, g, o.x0, o.x1, o.x2, Lx, Ly, Lz, S, lane);
    const bool active = t < f.n_terms;
    if (active) {
        long long* Fr = force + (size_t)r * 3 * Npad;
        if (f.kind == REMD_CUSTOM_EXTERNAL) add_force(Fr, Npad, o.a0, (float)-e.a, (float)-e.b, (float)-e.c);
        else {
            const double k = -e.a;
            add_force(Fr, Npad, o.a0, (float)(k * o.g0.x), (float)(k * o.g0.y), (float)(k * o.g0.z));
            add_force(Fr, Npad, o.a1, (float)(k * o.g1.x), (float)(k * o.g1.y), (float)(k * o.g1.z));
            if (f.kind != REMD_CUSTOM_BOND) add_force(Fr, Npad, o.a2, (float)(k * o.g2.x), (float)(k * o.g2.y), (float)(k * o.g2.z));
            if (f.kind == REMD_CUSTOM_TORSION) add_force(Fr, Npad, o.a3, (float)(k * o.g3.x), (float)(k * o.g3.y), (float)(k * o.g3.z));
        }
    }
    if (ENERGY) {
        const double ew = cst_wave_sum(active ? e.v : 0.0);
        if (lane == 0) Ewave[(size_t)r * waves + w] = ew;
    }
}

// grid (R), 64 threads: each force's wavefront partials in a fixed order -> E[r][f]; their sum joins the replica's energy partial
__global__ __launch_bounds__(64)
void custom_reduce_kernel(int nf, const cst_force* __restrict__ F, int waves, const double* __restrict__ Ewave, double* __restrict__ E,
                          double* __restrict__ epart, int n_epart, int ep_slot)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    double total = 0.0;
    for (int i = 0; i < nf; ++i) {
        const int w0 = F[i].slot0 / 64, nw = F[i].npad / 64;
        double e = 0.0;
        for (int w = lane; w < nw; w += 64) e += Ewave[(size_t)r * waves + w0 + w];
        e = cst_wave_sum(e);
        if (lane == 0) E[(size_t)r * nf + i] = e;
        total += e;
    }
    if (lane == 0) epart[(size_t)r * n_epart + ep_slot] += total;
}

// u_kl partials, grid (wavefronts, R): D[r][l][w] = sum over the wavefront's terms of e(g_l) - e(g_own), the difference formed per term
__global__ __launch_bounds__(64)
void custom_ukl_kernel(int total_pad, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ atoms,
                       const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                       const double* __restrict__ glob, int ng, int K, const int64_t* __restrict__ labels, int r_begin, int Npad,
                       const float4* __restrict__ pos, const float* __restrict__ box, double* __restrict__ D)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    const int w = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const float4* P = pos + (size_t)r * Npad;
    const double Lx = box[4 * r], Ly = box[4 * r + 1], Lz = box[4 * r + 2];
    const double* g_own = glob + (size_t)labels[r_begin + r] * ng;
    cst_geom o;
    cst_geometry(f, atoms, total_pad, s, P, Lx, Ly, Lz, o);
    const bool active = t < f.n_terms;
    double e_own = 0.0;
    for (int l = -1; l < K; ++l) {
        const double* g = l < 0 ? g_own : glob + (size_t)l * ng;
        bool same = l >= 0;
        for (int i = 0; i < ng && same; ++i) same = g[i] == g_own[i];
        double d = 0.0;
        if (!same) {
            const double e = cst_eval<false>(f, prog, consts, par, t, g, o.x0, o.x1, o.x2, Lx, Ly, Lz, S, lane).v;
            if (l < 0) e_own = e; else d = active ? e - e_own : 0.0;
        }
        if (l >= 0) {
            d = cst_wave_sum(d);
            if (lane == 0) D[((size_t)r * K + l) * waves + w] = d;
        }
    }
}

// grid (K, R), 64 threads: rows[r][l] += beta_l sum_w D[r][l][w], in a fixed order
__global__ __launch_bounds__(64)
void custom_ukl_reduce_kernel(int K, int waves, const double* __restrict__ D, const double* __restrict__ beta, double* __restrict__ rows)
{
    const int l = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    double d = 0.0;
    for (int w = lane; w < waves; w += 64) d += D[((size_t)r * K + l) * waves + w];
    d = cst_wave_sum(d);
    if (lane == 0) rows[(size_t)r * K + l] += beta[l] * d;
}

// energy parameter derivatives, grid (wavefronts of the four kinds' part, R): D[r][d][w] = sum over the wavefront's terms of
// dE/dglobal(dcols[d]) under the replica's own globals, the machine seeded at that column (cst_eval<., true>); a force whose mask lacks
// the column is skipped wave-uniformly and contributes exactly 0, and so do padding lanes.
// STATES (remd_get_custom_parameter_derivatives_at_states): the same under the globals of every state l in turn, D[r][l][d][w]; the
// geometry is computed once.  A compile-time switch: without it K is not read and the kernel is the code it was.
template <bool STATES>
__global__ __launch_bounds__(64)
void custom_dpar_kernel(int total_pad, int waves, const cst_force* __restrict__ F, const int* __restrict__ wave_force, const int* __restrict__ atoms,
                        const double* __restrict__ par, const int2* __restrict__ prog, const double* __restrict__ consts,
                        const double* __restrict__ glob, int ng, int nd, const int* __restrict__ dcols, const unsigned* __restrict__ dmask,
                        const int64_t* __restrict__ labels, int r_begin, int Npad, const float4* __restrict__ pos,
                        const float* __restrict__ box, double* __restrict__ D /*[R][nd][waves]; STATES: [R][K][nd][waves]*/, int K)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    const int w = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    const cst_force f = F[wave_force[w]];
    const unsigned mask = dmask[wave_force[w]];
    const int s = w * 64 + lane, t = s - f.slot0;
    const float4* P = pos + (size_t)r * Npad;
    const double Lx = box[4 * r], Ly = box[4 * r + 1], Lz = box[4 * r + 2];
    cst_geom o;
    cst_geometry(f, atoms, total_pad, s, P, Lx, Ly, Lz, o);
    const bool active = t < f.n_terms;
    const int nl = STATES ? K : 1;
    for (int l = 0; l < nl; ++l) {
        const double* g = glob + (size_t)(STATES ? l : labels[r_begin + r]) * ng;
        for (int d = 0; d < nd; ++d) {
            double v = 0.0;
            if ((mask >> d) & 1u) {
                const cx e = cst_eval<false, true>(f, prog, consts, par, t, g, o.x0, o.x1, o.x2, Lx, Ly, Lz, S, lane, nullptr, -1, dcols[d]);
                v = cst_wave_sum(active ? e.a : 0.0);
            }
            if (lane == 0) D[(((size_t)r * nl + l) * nd + d) * waves + w] = v;
        }
    }
}

// grid (nd, R), 64 threads: out[r][d] = sum_w D[r][d][w], in a fixed order (at every state: the rows are the R K pairs (r, l))
__global__ __launch_bounds__(64)
void custom_dpar_reduce_kernel(int nd, int waves, const double* __restrict__ D, double* __restrict__ out)
{
    const int d = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    double v = 0.0;
    for (int w = lane; w < waves; w += 64) v += D[((size_t)r * nd + d) * waves + w];
    v = cst_wave_sum(v);
    if (lane == 0) out[(size_t)r * nd + d] = v;
}

int ensure_buffers(remd_ctx* h, cst_tables& t)
{
    const size_t waves = (size_t)t.total_pad / 64;
    if (t.d_E.size() != (size_t)h->R * t.nf) {
        REMD_TRY(t.d_E.alloc(h, (size_t)h->R * t.nf));
        REMD_CHECK(h, hipMemset(t.d_E, 0, sizeof(double) * (size_t)h->R * t.nf));
    }
    if (t.d_Ewave.size() != (size_t)h->R * waves) REMD_TRY(t.d_Ewave.alloc(h, (size_t)h->R * waves));
    // centroid forces: the centroids and the gradients on them (a handle without such a force: n_groups = 0, nothing is allocated)
    const size_t nC = (size_t)h->R * t.n_groups * 3, nG = t.n_groups ? (size_t)h->R * (waves - t.begin(CST_CENTROID)) * 64 * REMD_CUSTOM_MAX_PARTICLES * 3 : 0;
    if (t.d_C.size() != nC) REMD_TRY(t.d_C.alloc(h, nC));
    if (t.d_G.size() != nG) REMD_TRY(t.d_G.alloc(h, nG));
    // collective-variable forces: what the superposition hands on (n_cv = 0: nothing is allocated)
    const size_t nW = (size_t)h->R * t.n_cv * remd_custom_cv_w();
    if (t.d_W.size() != nW) REMD_TRY(t.d_W.alloc(h, nW));
    // many-particle forces: the neighbour rows and their counts (mp_rows = 0: nothing is allocated)
    const size_t nR = (size_t)h->R * t.mp_rows;
    if (t.d_mp_cnt.size() != nR) REMD_TRY(t.d_mp_cnt.alloc(h, nR));
    if (t.d_mp_nbr.size() != nR * REMD_CUSTOM_MP_MAX_NEIGHBORS) REMD_TRY(t.d_mp_nbr.alloc(h, nR * REMD_CUSTOM_MP_MAX_NEIGHBORS));
    // Generalized-Born forces: partial sums, values and dE/dV (gb_work = 0: nothing is allocated)
    if (t.d_gb_work.size() != (size_t)h->R * t.gb_work) REMD_TRY(t.d_gb_work.alloc(h, (size_t)h->R * t.gb_work));
    return 0;
}

// the one list of the plan's tables: each to the device array of its name; the work buffers are forgotten (ensure_buffers)
int upload_tables(remd_ctx* h, cst_tables& t)
{
    int rc;
    // (the programs are int32 pairs on the host and int2 to the kernels)
    if ((rc = t.d_prog.alloc(h, t.prog.size() / 2))) return rc;
    if (!t.prog.empty()) REMD_CHECK(h, hipMemcpy(t.d_prog, t.prog.data(), sizeof(int) * t.prog.size(), hipMemcpyHostToDevice));
    if ((rc = t.d_F.upload(h, t.F)) || (rc = t.d_wave_force.upload(h, t.wave_force)) || (rc = t.d_atoms.upload(h, t.atoms)) ||
        (rc = t.d_par.upload(h, t.par)) || (rc = t.d_consts.upload(h, t.consts)) || (rc = t.d_glob.upload(h, t.glob)) ||
        (rc = t.d_grp_off.upload(h, t.grp_off)) || (rc = t.d_grp_atoms.upload(h, t.grp_atoms)) ||
        (rc = t.d_grp_w.upload(h, t.grp_w)) || (rc = t.d_grp_periodic.upload(h, t.grp_periodic)) || (rc = t.d_ref_off.upload(h, t.ref_off)) ||
        (rc = t.d_refs.upload(h, t.refs)) || (rc = t.d_excl_off.upload(h, t.excl_off)) || (rc = t.d_excl_atoms.upload(h, t.excl_atoms)) ||
        (rc = t.d_lrc.upload(h, t.lrc)) || (rc = t.d_mol_first.upload(h, t.mol_first)) || (rc = t.d_mol_size.upload(h, t.mol_size)) ||
        (rc = t.d_cv_off.upload(h, t.cv_off)) || (rc = t.d_cv_atoms.upload(h, t.cv_atoms)) || (rc = t.d_cv_ref.upload(h, t.cv_ref)) ||
        (rc = t.d_map_off.upload(h, t.map_off)) || (rc = t.d_map_index.upload(h, t.map_index)) ||
        (rc = t.d_hb_atoms.upload(h, t.hb_atoms)) || (rc = t.d_mp_types.upload(h, t.mp_types)) ||
        (rc = t.d_gb_stages.upload(h, t.gb_stages)) || (rc = t.d_dcols.upload(h, t.dcols)) || (rc = t.d_dmask.upload(h, t.dmask))) return rc;
    t.d_dD.reset(); t.d_dOut.reset(); t.d_dDK.reset(); t.d_dOutK.reset();
    t.d_E.reset(); t.d_Ewave.reset(); t.d_D.reset(); t.d_C.reset(); t.d_G.reset(); t.d_W.reset(); t.d_mp_nbr.reset(); t.d_mp_cnt.reset(); t.d_gb_work.reset();
    return 0;
}

bool globals_uniform(const cst_tables& t)
{
    for (int k = 1; k < t.K; ++k) for (int i = 0; i < t.ng; ++i) if (t.glob[(size_t)k * t.ng + i] != t.glob[i]) return false;
    return true;
}

// what a launch refuses to act on: globals of an older set of states, coefficients older than the globals
int check_current(remd_ctx* h, const cst_tables& t)
{
    if (t.K != h->K || t.glob_version != h->states_version)
        return remd_fail(h, -1, "custom terms: the states changed since remd_set_custom_globals (call it after remd_set_states)");
    if (t.has_lrc && !t.lrc_valid)
        return remd_fail(h, -1, "custom terms: a nonbonded force has a long-range correction and the globals changed since remd_set_custom_lrc (call it after remd_set_custom_globals)");
    return 0;
}

}  // namespace

int remd_custom_molecules(remd_ctx* h, const int** first, const int** size)
{
    cst_tables* t = h->cst.get();
    if (!t || h->n_custom == 0 || t->mol_first.empty()) return 0;
    *first = t->d_mol_first; *size = t->d_mol_size;
    return (int)t->mol_first.size();
}

void remd_custom_release(remd_ctx* h)
{
    if (h->cst) { hipStreamSynchronize(h->stream); if (h->stream2) hipStreamSynchronize(h->stream2); h->cst.reset(); }
    h->n_custom = 0; h->cst_group = 0; h->cst_cutoff = 0.0;
}

int remd_custom_clone(remd_ctx* parent, remd_ctx* child)
{
    const cst_tables* t = parent->cst.get();
    if (!t || parent->n_custom == 0) return 0;
    child->cst.reset(new cst_tables());
    cst_tables& c = *child->cst;
    static_cast<cst_plan&>(c) = *t;                     // the plan as a whole: whatever tables it has
    c.glob_version = t->glob_version == parent->states_version ? child->states_version : -1;
    hipSetDevice(child->device);
    const int rc = upload_tables(child, c);
    if (rc) return remd_fail(parent, rc, std::string("phases: ") + child->err);
    child->n_custom = parent->n_custom; child->cst_group = parent->cst_group; child->cst_cutoff = parent->cst_cutoff;
    child->config_version++;
    return 0;
}

// the custom terms' launch of a force evaluation (forces.hip: beside the restraints, on the stream of the listed terms)
int remd_custom_forces(remd_ctx* h, bool with_energy, int ep_slot, hipStream_t st)
{
    cst_tables* tp = h->cst.get();
    if (!tp || h->n_custom == 0) return 0;
    cst_tables& t = *tp;
    REMD_TRY(check_current(h, t));
    int rc = ensure_buffers(h, t); if (rc) return rc;
    const int waves = t.total_pad / 64;
    remd_prof_scope ps(h, "custom_terms", st);
    if (t.has(CST_SIMPLE)) {                             // (the first part: its wavefronts start at 0)
        if (with_energy)
            hipLaunchKernelGGL(custom_terms_kernel<true>, dim3(t.end(CST_SIMPLE), h->R), dim3(64), 0, st, t.total_pad, waves, t.d_F,
                               t.d_wave_force, t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, h->Npad, h->d_pos,
                               h->d_box, h->d_force, t.d_Ewave);
        else
            hipLaunchKernelGGL(custom_terms_kernel<false>, dim3(t.end(CST_SIMPLE), h->R), dim3(64), 0, st, t.total_pad, waves, t.d_F,
                               t.d_wave_force, t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, h->Npad, h->d_pos,
                               h->d_box, h->d_force, t.d_Ewave);
    }
    if (t.has(CST_COMPOUND)) remd_custom_compound_forces(h, t, with_energy, st);      // (each in the file of its kind, on its own part)
    if (t.has(CST_NONBONDED)) remd_custom_nonbonded_forces(h, t, with_energy, st);
    if (t.has(CST_CENTROID)) remd_custom_centroid_forces(h, t, with_energy, st);
    if (t.has(CST_CV)) remd_custom_cv_forces(h, t, with_energy, st);
    if (t.has(CST_CMAP)) remd_cmap_forces(h, t, with_energy, st);
    if (t.has(CST_HBOND)) remd_custom_hbond_forces(h, t, with_energy, st);
    if (t.has(CST_MANYPARTICLE)) remd_custom_manyparticle_forces(h, t, with_energy, st);
    if (t.has(CST_GB)) remd_custom_gb_forces(h, t, with_energy, st);
    if (with_energy)
        hipLaunchKernelGGL(custom_reduce_kernel, dim3(h->R), dim3(64), 0, st, t.nf, t.d_F, waves, t.d_Ewave, t.d_E, h->d_epart, h->n_epart, ep_slot);
    if (with_energy && t.has_lrc) remd_custom_nonbonded_lrc(h, t, ep_slot, st);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

// the custom terms' share of the u_kl rows, added to what the assembly wrote (behind the energy evaluation on the main stream)
int remd_custom_ukl(remd_ctx* h, double* d_rows)
{
    cst_tables* tp = h->cst.get();
    if (!tp || h->n_custom == 0) return 0;
    cst_tables& t = *tp;
    REMD_TRY(check_current(h, t));
    if (t.uniform) return 0;                          // every state carries the same globals: the share is exactly zero
    const int waves = t.total_pad / 64;
    const size_t nD = (size_t)h->R * h->K * waves;
    if (t.d_D.size() != nD) {
        // (the CMAP and Generalized-Born forces' wavefronts have no globals and no u_kl launch: their columns are zeroed here, once, and nothing writes them)
        REMD_TRY(t.d_D.alloc(h, nD));
        if (t.has(CST_CMAP) || t.has(CST_GB)) REMD_CHECK(h, hipMemsetAsync(t.d_D, 0, sizeof(double) * nD, h->stream));
    }
    remd_prof_scope ps(h, "custom_ukl");
    if (t.has(CST_SIMPLE))
        hipLaunchKernelGGL(custom_ukl_kernel, dim3(t.end(CST_SIMPLE), h->R), dim3(64), 0, h->stream, t.total_pad, waves, t.d_F, t.d_wave_force,
                           t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->K, h->d_labels, h->r_begin, h->Npad, h->d_pos, h->d_box, t.d_D);
    if (t.has(CST_COMPOUND)) remd_custom_compound_ukl(h, t);
    if (t.has(CST_NONBONDED)) remd_custom_nonbonded_ukl(h, t);
    if (t.has(CST_CENTROID)) remd_custom_centroid_ukl(h, t);
    if (t.has(CST_CV)) remd_custom_cv_ukl(h, t);
    if (t.has(CST_HBOND)) remd_custom_hbond_ukl(h, t);
    if (t.has(CST_MANYPARTICLE)) { REMD_TRY(ensure_buffers(h, t)); remd_custom_manyparticle_ukl(h, t); }
    hipLaunchKernelGGL(custom_ukl_reduce_kernel, dim3(h->K, h->R), dim3(64), 0, h->stream, h->K, waves, t.d_D, h->d_beta, d_rows);
    if (t.has_lrc) remd_custom_nonbonded_lrc_ukl(h, t, d_rows);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

// the kinds whose launches know the derivative mode (include/remd_hip_custom.h)
static bool dpar_served(int kind)
{
    return kind == REMD_CUSTOM_BOND || kind == REMD_CUSTOM_ANGLE || kind == REMD_CUSTOM_TORSION || kind == REMD_CUSTOM_EXTERNAL ||
           kind == REMD_CUSTOM_COMPOUND || kind == REMD_CUSTOM_CENTROID || kind == REMD_CUSTOM_HBOND || kind == REMD_CUSTOM_MANYPARTICLE;
}

// dE/dglobal of the declared columns at the current positions and the replicas' own globals -> d_dOut [R][nd], on the main stream.
// It runs whatever the states' globals are: a derivative does not vanish where every state carries the same ones.
// states: under every state's globals instead -> d_dOutK [R][K][nd], through partials of their own (d_dDK), so that the own-state
// call's buffers are what they were.  The staging launches (centroids, neighbour rows) run once either way.
static int remd_custom_dpar(remd_ctx* h, cst_tables& t, bool states)
{
    REMD_TRY(check_current(h, t));
    REMD_TRY(ensure_buffers(h, t));                     // (the centroids and the neighbour rows of the staging launches)
    REMD_TRY(remd_vsites_place(h, h->stream));
    const int waves = t.total_pad / 64, nd = (int)t.dcols.size();
    const size_t rows = (size_t)h->R * (states ? h->K : 1), nD = rows * nd * waves;
    if (rows > 65535) return remd_fail(h, -1, "custom terms: more than 65535 (replica, state) pairs in one energy parameter derivative call");
    dev_array<double>& dD = states ? t.d_dDK : t.d_dD;
    dev_array<double>& dOut = states ? t.d_dOutK : t.d_dOut;
    if (dD.size() != nD) {
        // (the wavefronts of the kinds that are not served are never written: zeroed here, once)
        REMD_TRY(dD.alloc(h, nD));
        REMD_CHECK(h, hipMemsetAsync(dD, 0, sizeof(double) * nD, h->stream));
    }
    if (dOut.size() != rows * nd) REMD_TRY(dOut.alloc(h, rows * nd));
    remd_prof_scope ps(h, states ? "custom_dpar_states" : "custom_dpar");
    if (t.has(CST_SIMPLE)) {
        if (states)
            hipLaunchKernelGGL(custom_dpar_kernel<true>, dim3(t.end(CST_SIMPLE), h->R), dim3(64), 0, h->stream, t.total_pad, waves, t.d_F, t.d_wave_force,
                               t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, nd, t.d_dcols, t.d_dmask, h->d_labels, h->r_begin, h->Npad,
                               h->d_pos, h->d_box, dD, h->K);
        else
            hipLaunchKernelGGL(custom_dpar_kernel<false>, dim3(t.end(CST_SIMPLE), h->R), dim3(64), 0, h->stream, t.total_pad, waves, t.d_F, t.d_wave_force,
                               t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, nd, t.d_dcols, t.d_dmask, h->d_labels, h->r_begin, h->Npad,
                               h->d_pos, h->d_box, dD, 1);
    }
    if (t.has(CST_COMPOUND)) remd_custom_compound_dpar(h, t, states);
    if (t.has(CST_CENTROID)) remd_custom_centroid_dpar(h, t, states);
    if (t.has(CST_HBOND)) remd_custom_hbond_dpar(h, t, states);
    if (t.has(CST_MANYPARTICLE)) remd_custom_manyparticle_dpar(h, t, states);
    hipLaunchKernelGGL(custom_dpar_reduce_kernel, dim3(nd, (unsigned)rows), dim3(64), 0, h->stream, nd, waves, dD, dOut);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

extern "C" {

int remd_set_custom_parameter_derivatives(remd_handle h, const int32_t* columns, int n, const uint32_t* force_masks)
{
    if (!h || n < 0 || (n > 0 && (!columns || !force_masks))) return remd_fail(h, -1, "remd_set_custom_parameter_derivatives: bad arguments");
    cst_tables* t = h->cst.get();
    if (!t || h->n_custom == 0) return remd_fail(h, -1, "remd_set_custom_parameter_derivatives: no custom terms (remd_set_custom_terms)");
    if (n > REMD_CUSTOM_MAX_GLOBALS) return remd_fail(h, -1, "remd_set_custom_parameter_derivatives: more than REMD_CUSTOM_MAX_GLOBALS derivatives");
    for (int d = 0; d < n; ++d) {
        if (columns[d] < 0 || columns[d] >= t->ng) return remd_fail(h, -1, "remd_set_custom_parameter_derivatives: a global-parameter column out of range");
        for (int e = 0; e < d; ++e)
            if (columns[e] == columns[d]) return remd_fail(h, -1, "remd_set_custom_parameter_derivatives: a global-parameter column named twice");
    }
    for (int i = 0; i < t->nf && n > 0; ++i) {
        if (n < 32 && (force_masks[i] >> n) != 0u) return remd_fail(h, -1, "remd_set_custom_parameter_derivatives: a mask bit beyond the listed columns");
        if (force_masks[i] != 0u && !dpar_served(t->F[i].kind))
            return remd_fail(h, -1, "remd_set_custom_parameter_derivatives: force " + std::to_string(i) + " is of a kind without energy parameter derivatives "
                                    "(nonbonded, collective-variable, CMAP and Generalized-Born forces have none)");
    }
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    if (h->stream2) hipStreamSynchronize(h->stream2);
    t->dcols.assign(columns, columns + n);
    if (n > 0) t->dmask.assign(force_masks, force_masks + t->nf); else t->dmask.clear();
    t->d_dD.reset(); t->d_dOut.reset(); t->d_dDK.reset(); t->d_dOutK.reset();
    int rc;
    if ((rc = t->d_dcols.upload(h, t->dcols)) || (rc = t->d_dmask.upload(h, t->dmask))) return rc;
    h->config_version++;
    return 0;
}

int remd_get_custom_parameter_derivatives(remd_handle h, double* out)
{
    if (!h || !out || h->R <= 0) return remd_fail(h, -1, "remd_get_custom_parameter_derivatives: bad arguments");
    cst_tables* t = h->cst.get();
    if (!t || h->n_custom == 0 || t->dcols.empty())
        return remd_fail(h, -1, "remd_get_custom_parameter_derivatives: no energy parameter derivative declared (remd_set_custom_parameter_derivatives)");
    hipSetDevice(h->device);
    int rc = remd_custom_dpar(h, *t, false); if (rc) return rc;
    REMD_CHECK(h, hipMemcpyAsync(out, t->d_dOut, sizeof(double) * (size_t)h->R * t->dcols.size(), hipMemcpyDeviceToHost, h->stream));
    REMD_CHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int remd_get_custom_parameter_derivatives_at_states(remd_handle h, double* out)
{
    if (!h || !out) return remd_fail(h, -1, "remd_get_custom_parameter_derivatives_at_states: bad arguments");
    if (h->R <= 0) return remd_fail(h, -1, "remd_get_custom_parameter_derivatives_at_states: no replicas (remd_set_replicas)");
    cst_tables* t = h->cst.get();
    if (!t || h->n_custom == 0 || t->dcols.empty())
        return remd_fail(h, -1, "remd_get_custom_parameter_derivatives_at_states: no energy parameter derivative declared (remd_set_custom_parameter_derivatives)");
    if (h->K <= 0) return remd_fail(h, -1, "remd_get_custom_parameter_derivatives_at_states: no states (remd_set_states, then remd_set_custom_globals)");
    hipSetDevice(h->device);
    int rc = remd_custom_dpar(h, *t, true); if (rc) return rc;
    REMD_CHECK(h, hipMemcpyAsync(out, t->d_dOutK, sizeof(double) * (size_t)h->R * h->K * t->dcols.size(), hipMemcpyDeviceToHost, h->stream));
    REMD_CHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int remd_set_custom_terms(remd_handle h, const remd_custom_force_desc* desc, int n)
{
    if (!h || n < 0 || (n > 0 && !desc)) return remd_fail(h, -1, "remd_set_custom_terms: bad arguments");
    if (!h->has_system) return remd_fail(h, -1, "remd_set_custom_terms: call remd_set_system first");
    hipSetDevice(h->device);
    if (n == 0) { remd_custom_release(h); h->config_version++; return 0; }
    // (the planner only fills `t` and touches nothing of the handle or the device: a refused call leaves the handle as it was)
    const bool bare = h->nb_method == REMD_NB_NONE && !h->nocutoff && h->n_bonds + h->n_angles + h->n_torsions + h->n_settle + h->n_shake == 0;
    const cst_facts facts{h->N, h->Npad, h->K, h->states_version, h->box_host.data(), h->box_host.size(), bare};
    cst_tables t;
    const std::string refusal = cst_build_plan(desc, n, facts, t);
    if (!refusal.empty()) return remd_fail(h, -1, "remd_set_custom_terms: " + refusal);
    remd_custom_release(h);
    h->config_version++;
    int rc = upload_tables(h, t);
    if (rc) return rc;
    const double periodic_cutoff = t.periodic_cutoff;
    h->cst.reset(new cst_tables(std::move(t)));
    h->n_custom = n; h->cst_group = desc[0].force_group; h->cst_cutoff = periodic_cutoff;
    return 0;
}

int remd_set_custom_globals(remd_handle h, const double* values)
{
    if (!h) return remd_fail(h, -1, "remd_set_custom_globals: bad arguments");
    cst_tables* t = h->cst.get();
    if (!t || h->n_custom == 0) return remd_fail(h, -1, "remd_set_custom_globals: no custom terms (remd_set_custom_terms)");
    if (h->K <= 0) return remd_fail(h, -1, "remd_set_custom_globals: call remd_set_states first");
    if (t->ng > 0 && !values) return remd_fail(h, -1, "remd_set_custom_globals: bad arguments");
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    if (h->stream2) hipStreamSynchronize(h->stream2);
    t->K = h->K; t->glob_version = h->states_version;
    if (t->ng > 0) t->glob.assign(values, values + (size_t)h->K * t->ng); else t->glob.assign(1, 0.0);
    t->uniform = t->ng == 0 || globals_uniform(*t);
    t->lrc_valid = false;                               // (the coefficients are integrals of the expressions under the globals)
    int rc = t->d_glob.upload(h, t->glob);
    if (rc) return rc;
    h->config_version++;
    return 0;
}

int remd_set_custom_lrc(remd_handle h, const double* coeff)
{
    if (!h) return remd_fail(h, -1, "remd_set_custom_lrc: bad arguments");
    cst_tables* t = h->cst.get();
    if (!t || h->n_custom == 0) return remd_fail(h, -1, "remd_set_custom_lrc: no custom terms (remd_set_custom_terms)");
    if (h->K <= 0 || t->K != h->K || t->glob_version != h->states_version)
        return remd_fail(h, -1, "remd_set_custom_lrc: call remd_set_states and remd_set_custom_globals first");
    if (!coeff) return remd_fail(h, -1, "remd_set_custom_lrc: bad arguments");
    for (size_t k = 0; k < (size_t)h->K * t->nf; ++k)
        if (!std::isfinite(coeff[k]) || (coeff[k] != 0.0 && !t->F[k % t->nf].lrc))
            return remd_fail(h, -1, "remd_set_custom_lrc: a coefficient that is not finite, or not zero for a force without a long-range correction");
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    if (h->stream2) hipStreamSynchronize(h->stream2);
    t->lrc.assign(coeff, coeff + (size_t)h->K * t->nf);
    int rc = t->d_lrc.upload(h, t->lrc);
    if (rc) return rc;
    t->lrc_valid = true;
    h->config_version++;
    h->forces_valid = false;
    return 0;
}

int remd_get_custom_energies(remd_handle h, double* out)
{
    if (!h || !out || h->R <= 0) return remd_fail(h, -1, "remd_get_custom_energies: bad arguments");
    cst_tables* t = h->cst.get();
    if (!t || h->n_custom == 0) return remd_fail(h, -1, "remd_get_custom_energies: no custom terms (remd_set_custom_terms)");
    hipSetDevice(h->device);
    int rc = remd_compute_forces(h, true); if (rc) return rc;
    REMD_CHECK(h, hipMemcpyAsync(out, t->d_E, sizeof(double) * (size_t)h->R * t->nf, hipMemcpyDeviceToHost, h->stream));
    REMD_CHECK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int remd_get_custom_cv_values(remd_handle h, double* out)
{
    if (!h || !out || h->R <= 0) return remd_fail(h, -1, "remd_get_custom_cv_values: bad arguments");
    cst_tables* t = h->cst.get();
    if (!t || h->n_custom == 0 || t->n_cv == 0) return remd_fail(h, -1, "remd_get_custom_cv_values: no collective-variable force (remd_set_custom_terms)");
    hipSetDevice(h->device);
    int rc = remd_compute_forces(h, true); if (rc) return rc;
    const size_t w = remd_custom_cv_w(), n = (size_t)h->R * t->n_cv;
    std::vector<double> W(n * w);
    REMD_CHECK(h, hipMemcpyAsync(W.data(), t->d_W, sizeof(double) * n * w, hipMemcpyDeviceToHost, h->stream));
    REMD_CHECK(h, hipStreamSynchronize(h->stream));
    for (size_t k = 0; k < n; ++k) out[k] = W[k * w];
    return 0;
}

}  // extern "C"
