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
// comes last and runs no program: it shares the term space, the tables and the energy reduction only.
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

int ensure_buffers(remd_ctx* h, cst_tables& t)
{
    const size_t waves = (size_t)t.total_pad / 64;
    if (t.d_E.size() != (size_t)h->R * t.nf) {
        REMD_TRY(t.d_E.alloc(h, (size_t)h->R * t.nf));
        REMD_CHECK(h, hipMemset(t.d_E, 0, sizeof(double) * (size_t)h->R * t.nf));
    }
    if (t.d_Ewave.size() != (size_t)h->R * waves) REMD_TRY(t.d_Ewave.alloc(h, (size_t)h->R * waves));
    // centroid forces: the centroids and the gradients on them (a handle without such a force: n_groups = 0, nothing is allocated)
    const size_t nC = (size_t)h->R * t.n_groups * 3, nG = (size_t)h->R * (waves - t.waves_particles) * 64 * REMD_CUSTOM_MAX_PARTICLES * 3;
    if (t.d_C.size() != nC) REMD_TRY(t.d_C.alloc(h, nC));
    if (t.d_G.size() != nG) REMD_TRY(t.d_G.alloc(h, nG));
    // collective-variable forces: what the superposition hands on (n_cv = 0: nothing is allocated)
    const size_t nW = (size_t)h->R * t.n_cv * remd_custom_cv_w();
    if (t.d_W.size() != nW) REMD_TRY(t.d_W.alloc(h, nW));
    return 0;
}

int set_tables(remd_ctx* h, cst_tables& t)
{
    int rc;
    if ((rc = t.d_F.upload(h, t.F)) || (rc = t.d_wave_force.upload(h, t.wave_force)) || (rc = t.d_atoms.upload(h, t.atoms)) ||
        (rc = t.d_par.upload(h, t.par)) || (rc = t.d_consts.upload(h, t.consts)) || (rc = t.d_glob.upload(h, t.glob)) ||
        (rc = t.d_prog.upload(h, t.prog)) || (rc = t.d_grp_off.upload(h, t.grp_off)) || (rc = t.d_grp_atoms.upload(h, t.grp_atoms)) ||
        (rc = t.d_grp_w.upload(h, t.grp_w)) || (rc = t.d_grp_periodic.upload(h, t.grp_periodic)) || (rc = t.d_ref_off.upload(h, t.ref_off)) ||
        (rc = t.d_refs.upload(h, t.refs)) || (rc = t.d_excl_off.upload(h, t.excl_off)) || (rc = t.d_excl_atoms.upload(h, t.excl_atoms)) ||
        (rc = t.d_lrc.upload(h, t.lrc)) || (rc = t.d_mol_first.upload(h, t.mol_first)) || (rc = t.d_mol_size.upload(h, t.mol_size)) ||
        (rc = t.d_cv_off.upload(h, t.cv_off)) || (rc = t.d_cv_atoms.upload(h, t.cv_atoms)) || (rc = t.d_cv_ref.upload(h, t.cv_ref)) ||
        (rc = t.d_map_off.upload(h, t.map_off)) || (rc = t.d_map_index.upload(h, t.map_index))) return rc;
    t.d_E.reset(); t.d_Ewave.reset(); t.d_D.reset(); t.d_C.reset(); t.d_G.reset(); t.d_W.reset();
    return 0;
}

bool globals_uniform(const cst_tables& t)
{
    for (int k = 1; k < t.K; ++k) for (int i = 0; i < t.ng; ++i) if (t.glob[(size_t)k * t.ng + i] != t.glob[i]) return false;
    return true;
}

// what a program may do is settled here, once: the kernels index the stack, the constants, the parameters and the globals unchecked
const char* check_program(const remd_custom_force_desc& d, int n_vars)
{
    const bool compound = d.kind == REMD_CUSTOM_COMPOUND || d.kind == REMD_CUSTOM_CENTROID;
    const int n_par = d.kind == REMD_CUSTOM_NONBONDED ? 2 * d.n_params : d.n_params;     // (a pair: particle 1's parameters, then particle 2's)
    if (d.n_program <= 0 || !d.program) return "an empty program";
    if (d.n_program > REMD_CUSTOM_MAX_PROGRAM) return "a program over REMD_CUSTOM_MAX_PROGRAM instructions";
    int sp = 0, top = 0;
    for (int pc = 0; pc < d.n_program; ++pc) {
        const int op = d.program[2 * pc], arg = d.program[2 * pc + 1];
        int pops = 1;
        switch (op) {
        case REMD_CX_CONST:  if (arg < 0 || arg >= d.n_consts || !d.consts) return "a constant index out of range"; pops = 0; break;
        case REMD_CX_VAR:    if (arg < 0 || arg >= n_vars) return "a variable index out of range"; pops = 0; break;
        case REMD_CX_PARAM:  if (arg < 0 || arg >= n_par) return "a parameter index out of range"; pops = 0; break;
        case REMD_CX_GLOBAL: if (arg < 0 || arg >= d.n_globals) return "a global-parameter index out of range"; pops = 0; break;
        case REMD_CX_ADD: case REMD_CX_SUB: case REMD_CX_MUL: case REMD_CX_DIV: case REMD_CX_POW: case REMD_CX_ATAN2:
        case REMD_CX_MIN: case REMD_CX_MAX: pops = 2; break;
        case REMD_CX_SELECT: pops = 3; break;
        case REMD_CX_PERIODICDISTANCE: pops = 6; break;
        case REMD_CX_DISTANCE: case REMD_CX_ANGLE: case REMD_CX_DIHEDRAL: {
            // the zero-based particle slots in 4-bit fields, first argument lowest; nothing above them
            if (!compound) return "a function of particles outside a compound-bond or centroid-bond force";
            const int n_args = op - REMD_CX_DISTANCE + 2;
            if (arg < 0 || (arg >> (4 * n_args)) != 0) return "a particle slot out of range";
            for (int k = 0; k < n_args; ++k) if (((arg >> (4 * k)) & 15) >= d.n_particles) return "a particle slot out of range";
            pops = 0;
        } break;
        case REMD_CX_POWI: if (arg < -64 || arg > 64) return "an integer power beyond +-64"; break;
        case REMD_CX_TABLE1D: case REMD_CX_LOOKUP1D: {
            // the block of the function at consts[arg] (include/remd_hip_custom.h): the kernels trust n, min, max and the block's extent
            const bool spline = op == REMD_CX_TABLE1D;
            if (arg < 0 || arg >= d.n_consts || !d.consts) return "a table offset out of range";
            const double n = d.consts[arg];
            if (!(n >= (spline ? 2.0 : 1.0) && n <= (double)REMD_CUSTOM_MAX_TABLE_POINTS) || n != floor(n))
                return spline ? "a table whose point count is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_POINTS"
                              : "a lookup table whose value count is not an integer 1 ... REMD_CUSTOM_MAX_TABLE_POINTS";
            if ((long long)arg + (spline ? 4 + 2 * (long long)n : 1 + (long long)n) > (long long)d.n_consts) return "a table that runs past n_consts";
            if (spline) {
                const double lo = d.consts[arg + 1], hi = d.consts[arg + 2], periodic = d.consts[arg + 3];
                if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return "a table whose bounds are not finite with min < max";
                if (periodic != 0.0 && periodic != 1.0) return "a table whose periodic flag is neither 0 nor 1";
            }
        } break;
        case REMD_CX_TABLE2D: case REMD_CX_LOOKUP2D: case REMD_CX_LOOKUP3D: {
            // the same for the blocks of two and three arguments: the sizes, their product, the bounds and the extent
            const bool patch = op == REMD_CX_TABLE2D;
            const int dims = op == REMD_CX_LOOKUP3D ? 3 : 2, header = patch ? 8 : dims == 3 ? 4 : 2;
            if (arg < 0 || arg >= d.n_consts || !d.consts) return "a table offset out of range";
            if ((long long)arg + header > (long long)d.n_consts) return "a table that runs past n_consts";
            double cells = 1.0;
            for (int k = 0; k < dims; ++k) {
                const double n = d.consts[arg + k];
                if (!(n >= (patch ? 2.0 : 1.0) && n <= (double)REMD_CUSTOM_MAX_TABLE_CELLS) || n != floor(n))
                    return patch ? "a 2D table whose size is not an integer 2 ... REMD_CUSTOM_MAX_TABLE_CELLS"
                                 : "a lookup table whose size is not an integer 1 ... REMD_CUSTOM_MAX_TABLE_CELLS";
                cells *= n;
            }
            if (cells > (double)REMD_CUSTOM_MAX_TABLE_CELLS) return "a table of more than REMD_CUSTOM_MAX_TABLE_CELLS cells";
            if ((long long)arg + header + (patch ? 4 : 1) * (long long)cells > (long long)d.n_consts) return "a table that runs past n_consts";
            if (patch) {
                for (int k = 0; k < 2; ++k) {
                    const double lo = d.consts[arg + 2 + 2 * k], hi = d.consts[arg + 3 + 2 * k];
                    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return "a table whose bounds are not finite with min < max";
                }
                if (d.consts[arg + 6] != 0.0 && d.consts[arg + 6] != 1.0) return "a table whose periodic flag is neither 0 nor 1";
            }
            pops = dims;
        } break;
        default: if (op < 0 || op >= REMD_CX_N_OPCODES) return "an unknown opcode"; break;
        }
        if (sp < pops) return "a program that pops an empty stack";
        sp += 1 - pops;
        top = std::max(top, sp);
        if (sp > REMD_CUSTOM_MAX_STACK) return "a program over REMD_CUSTOM_MAX_STACK stack slots";
    }
    if (sp != 1) return "a program that does not leave exactly one value";
    if (top != d.stack_depth) return "a stack depth that is not the program's";
    return nullptr;
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
    c.nf = t->nf; c.ng = t->ng; c.K = t->K; c.total_pad = t->total_pad; c.waves_simple = t->waves_simple; c.uniform = t->uniform;
    c.waves_particles = t->waves_particles; c.n_groups = t->n_groups; c.waves_compound = t->waves_compound;
    c.excl_off = t->excl_off; c.excl_atoms = t->excl_atoms; c.lrc = t->lrc; c.has_lrc = t->has_lrc; c.lrc_valid = t->lrc_valid; c.periodic_cutoff = t->periodic_cutoff;
    c.mol_first = t->mol_first; c.mol_size = t->mol_size;
    c.waves_centroid = t->waves_centroid; c.n_cv = t->n_cv; c.cv_off = t->cv_off; c.cv_atoms = t->cv_atoms; c.cv_ref = t->cv_ref;
    c.waves_cv = t->waves_cv; c.map_off = t->map_off; c.map_index = t->map_index;
    c.grp_off = t->grp_off; c.grp_atoms = t->grp_atoms; c.grp_w = t->grp_w; c.grp_periodic = t->grp_periodic; c.ref_off = t->ref_off; c.refs = t->refs;
    c.glob_version = t->glob_version == parent->states_version ? child->states_version : -1;
    c.F = t->F; c.wave_force = t->wave_force; c.atoms = t->atoms; c.par = t->par; c.consts = t->consts; c.glob = t->glob;
    c.defaults = t->defaults; c.prog = t->prog;
    hipSetDevice(child->device);
    const int rc = set_tables(child, c);
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
    if (t.K != h->K || t.glob_version != h->states_version)
        return remd_fail(h, -1, "custom terms: the states changed since remd_set_custom_globals (call it after remd_set_states)");
    if (t.has_lrc && !t.lrc_valid)
        return remd_fail(h, -1, "custom terms: a nonbonded force has a long-range correction and the globals changed since remd_set_custom_lrc (call it after remd_set_custom_globals)");
    int rc = ensure_buffers(h, t); if (rc) return rc;
    const int waves = t.total_pad / 64;
    remd_prof_scope ps(h, "custom_terms", st);
    if (t.waves_simple > 0) {
        if (with_energy)
            hipLaunchKernelGGL(custom_terms_kernel<true>, dim3(t.waves_simple, h->R), dim3(64), 0, st, t.total_pad, waves, t.d_F,
                               t.d_wave_force, t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, h->Npad, h->d_pos,
                               h->d_box, h->d_force, t.d_Ewave);
        else
            hipLaunchKernelGGL(custom_terms_kernel<false>, dim3(t.waves_simple, h->R), dim3(64), 0, st, t.total_pad, waves, t.d_F,
                               t.d_wave_force, t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->d_labels, h->r_begin, h->Npad, h->d_pos,
                               h->d_box, h->d_force, t.d_Ewave);
    }
    if (t.waves_compound > t.waves_simple) remd_custom_compound_forces(h, t, with_energy, st);    // (custom_compound.hip: the wavefronts behind)
    if (t.waves_particles > t.waves_compound) remd_custom_nonbonded_forces(h, t, with_energy, st); // (custom_nonbonded.hip: the tiles behind those)
    if (t.waves_centroid > t.waves_particles) remd_custom_centroid_forces(h, t, with_energy, st);  // (custom_centroid.hip: behind those)
    if (t.waves_cv > t.waves_centroid) remd_custom_cv_forces(h, t, with_energy, st);               // (custom_cv.hip: behind those)
    if (waves > t.waves_cv) remd_cmap_forces(h, t, with_energy, st);                               // (cmap.hip: the last ones)
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
    if (t.K != h->K || t.glob_version != h->states_version)
        return remd_fail(h, -1, "custom terms: the states changed since remd_set_custom_globals (call it after remd_set_states)");
    if (t.has_lrc && !t.lrc_valid)
        return remd_fail(h, -1, "custom terms: a nonbonded force has a long-range correction and the globals changed since remd_set_custom_lrc (call it after remd_set_custom_globals)");
    if (t.uniform) return 0;                          // every state carries the same globals: the share is exactly zero
    const int waves = t.total_pad / 64;
    const size_t nD = (size_t)h->R * h->K * waves;
    if (t.d_D.size() != nD) {
        // (the CMAP forces' wavefronts have no globals and no u_kl launch: their columns are zeroed here, once, and nothing writes them)
        REMD_TRY(t.d_D.alloc(h, nD));
        if (waves > t.waves_cv) REMD_CHECK(h, hipMemsetAsync(t.d_D, 0, sizeof(double) * nD, h->stream));
    }
    remd_prof_scope ps(h, "custom_ukl");
    if (t.waves_simple > 0)
        hipLaunchKernelGGL(custom_ukl_kernel, dim3(t.waves_simple, h->R), dim3(64), 0, h->stream, t.total_pad, waves, t.d_F, t.d_wave_force,
                           t.d_atoms, t.d_par, t.d_prog, t.d_consts, t.d_glob, t.ng, h->K, h->d_labels, h->r_begin, h->Npad, h->d_pos, h->d_box, t.d_D);
    if (t.waves_compound > t.waves_simple) remd_custom_compound_ukl(h, t);
    if (t.waves_particles > t.waves_compound) remd_custom_nonbonded_ukl(h, t);
    if (t.waves_centroid > t.waves_particles) remd_custom_centroid_ukl(h, t);
    if (t.waves_cv > t.waves_centroid) remd_custom_cv_ukl(h, t);
    hipLaunchKernelGGL(custom_ukl_reduce_kernel, dim3(h->K, h->R), dim3(64), 0, h->stream, h->K, waves, t.d_D, h->d_beta, d_rows);
    if (t.has_lrc) remd_custom_nonbonded_lrc_ukl(h, t, d_rows);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

extern "C" {

int remd_set_custom_terms(remd_handle h, const remd_custom_force_desc* desc, int n)
{
    if (!h || n < 0 || (n > 0 && !desc)) return remd_fail(h, -1, "remd_set_custom_terms: bad arguments");
    if (!h->has_system) return remd_fail(h, -1, "remd_set_custom_terms: call remd_set_system first");
    hipSetDevice(h->device);
    if (n == 0) { remd_custom_release(h); h->config_version++; return 0; }
    // (everything below up to set_tables only fills `t`: a refused call leaves the handle as it was)
    if (n > REMD_CUSTOM_MAX_FORCES) return remd_fail(h, -1, "remd_set_custom_terms: more than REMD_CUSTOM_MAX_FORCES custom forces");
    cst_tables t;
    t.nf = n; t.ng = desc[0].n_globals;
    if (t.ng < 0 || t.ng > REMD_CUSTOM_MAX_GLOBALS) return remd_fail(h, -1, "remd_set_custom_terms: more than REMD_CUSTOM_MAX_GLOBALS global parameters");
    if (t.ng > 0 && !desc[0].global_defaults) return remd_fail(h, -1, "remd_set_custom_terms: global_defaults missing");
    t.defaults.assign(desc[0].global_defaults, desc[0].global_defaults + t.ng);
    static const int width4[4] = {2, 3, 4, 1}, n_vars4[4] = {1, 1, 1, 3};
    for (int i = 0; i < n; ++i) {
        const remd_custom_force_desc& d = desc[i];
        const std::string who = "remd_set_custom_terms: force " + std::to_string(i) + ": ";
        if (d.kind < 0 || d.kind > REMD_CUSTOM_CMAP) return remd_fail(h, -1, who + "unknown kind");
        const bool nonbonded = d.kind == REMD_CUSTOM_NONBONDED, cv = d.kind == REMD_CUSTOM_CV, cmap = d.kind == REMD_CUSTOM_CMAP;
        const bool centroid = d.kind == REMD_CUSTOM_CENTROID, compound = d.kind == REMD_CUSTOM_COMPOUND || centroid;
        if (cmap && d.n_particles != 8) return remd_fail(h, -1, who + "n_particles is 8 for a CMAP force (two dihedrals of four particles)");
        if (!cmap && (compound ? (d.n_particles < 1 || d.n_particles > REMD_CUSTOM_MAX_PARTICLES) : d.n_particles != 0))
            return remd_fail(h, -1, who + "n_particles is 1 ... REMD_CUSTOM_MAX_PARTICLES for a compound-bond or centroid-bond force and 0 for every other kind");
        const int wd = compound ? d.n_particles : cmap ? 8 : (nonbonded || cv) ? 0 : width4[d.kind];
        if (d.n_terms <= 0 || (!d.atoms && !nonbonded && !cv)) return remd_fail(h, -1, who + "no terms");
        if (d.n_params < 0 || d.n_params > REMD_CUSTOM_MAX_PARAMS || (d.n_params > 0 && !d.params))
            return remd_fail(h, -1, who + "0 ... REMD_CUSTOM_MAX_PARAMS parameters per term are supported");
        if (nonbonded) {
            // what custom_nonbonded.hip indexes unchecked: one parameter row per atom of the system, 2 n_params operands, the exclusion rows
            if (d.n_terms != h->N) return remd_fail(h, -1, who + "a nonbonded force has " + std::to_string(d.n_terms) + " particles, the system has " + std::to_string(h->N));
            if (2 * d.n_params > REMD_CUSTOM_MAX_PARAMS) return remd_fail(h, -1, who + "a nonbonded force takes at most REMD_CUSTOM_MAX_PARAMS / 2 per-particle parameters");
            if (d.nb_method < 0 || d.nb_method > 2) return remd_fail(h, -1, who + "unknown nonbonded method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic)");
            if ((d.periodic != 0) != (d.nb_method == 2)) return remd_fail(h, -1, who + "a nonbonded force is periodic exactly where its method is CutoffPeriodic");
            if (d.nb_method != 0 && !(d.cutoff > 0.0)) return remd_fail(h, -1, who + "a cutoff that is not positive");
            if (d.switch_distance >= 0.0 && (d.nb_method == 0 || !(d.switch_distance > 0.0 && d.switch_distance < d.cutoff)))
                return remd_fail(h, -1, who + "the switching distance must lie in (0, cutoff) and needs a cutoff");
            if (d.long_range_correction && d.nb_method != 2) return remd_fail(h, -1, who + "a long-range correction needs CutoffPeriodic");
            if (!d.excl_offsets || d.excl_offsets[0] != 0) return remd_fail(h, -1, who + "excl_offsets [N + 1] must start at 0");
            for (int a = 0; a < d.n_terms; ++a) {
                const int b = d.excl_offsets[a], e = d.excl_offsets[a + 1];
                if (e < b || (e > b && !d.excl_atoms)) return remd_fail(h, -1, who + "excl_offsets must not decrease");
                for (int k = b; k < e; ++k) {
                    if (d.excl_atoms[k] < 0 || d.excl_atoms[k] >= d.n_terms) return remd_fail(h, -1, who + "exclusion index out of range");
                    if (d.excl_atoms[k] == a) return remd_fail(h, -1, who + "a particle excluded from itself");
                }
            }
            if (d.nb_method == 2 && !h->box_host.empty())
                for (size_t k = 0; k < h->box_host.size(); ++k)
                    if (!(h->box_host[k] >= 2.0 * d.cutoff)) return remd_fail(h, -1, who + "box smaller than twice the cutoff");
        }
        if (cv) {
            // what custom_cv.hip indexes unchecked: the variables in CSR form, their particles, the reference beside them
            if (d.n_terms != 1 || d.n_params != 0 || d.periodic != 0) return remd_fail(h, -1, who + "a collective-variable force has n_terms = 1, no per-term parameters and is not periodic");
            if (d.n_cvs < 1 || d.n_cvs > REMD_CUSTOM_MAX_CVS) return remd_fail(h, -1, who + "a collective-variable force has 1 ... REMD_CUSTOM_MAX_CVS collective variables");
            if (!d.cv_offsets || !d.cv_atoms || !d.cv_reference) return remd_fail(h, -1, who + "a collective-variable force needs cv_offsets, cv_atoms and cv_reference");
            if (d.cv_offsets[0] != 0) return remd_fail(h, -1, who + "cv_offsets must start at 0");
            std::vector<char> seen(h->N);
            for (int c = 0; c < d.n_cvs; ++c) {
                const int b = d.cv_offsets[c], e = d.cv_offsets[c + 1];
                if (e < b || e - b < 3) return remd_fail(h, -1, who + "collective variable " + std::to_string(c) + ": an RMSD needs at least 3 particles");
                std::fill(seen.begin(), seen.end(), 0);
                double m[3] = {0.0, 0.0, 0.0};
                for (int k = b; k < e; ++k) {
                    const int a = d.cv_atoms[k];
                    if (a < 0 || a >= h->N) return remd_fail(h, -1, who + "collective variable " + std::to_string(c) + ": particle index out of range");
                    if (seen[a]) return remd_fail(h, -1, who + "collective variable " + std::to_string(c) + ": particle " + std::to_string(a) + " named twice");
                    seen[a] = 1;
                    for (int x = 0; x < 3; ++x) {
                        if (!std::isfinite(d.cv_reference[3 * (size_t)k + x])) return remd_fail(h, -1, who + "collective variable " + std::to_string(c) + ": a reference position that is not finite");
                        m[x] += d.cv_reference[3 * (size_t)k + x];
                    }
                }
                for (int x = 0; x < 3; ++x)
                    if (!(fabs(m[x]) <= 1e-9 * (e - b))) return remd_fail(h, -1, who + "collective variable " + std::to_string(c) + ": the reference must be centred on its own centroid (within 1e-9 nm)");
            }
        }
        if (cmap) {
            // what cmap.hip indexes unchecked: every term's map, every map's block (the header cst_table2d trusts, and its extent)
            if (d.n_params != 0 || d.n_program != 0) return remd_fail(h, -1, who + "a CMAP force has no per-term parameters and no program");
            if (d.n_maps < 1 || d.n_maps > REMD_CUSTOM_MAX_MAPS) return remd_fail(h, -1, who + "a CMAP force has 1 ... REMD_CUSTOM_MAX_MAPS maps");
            if (!d.map_index || !d.map_offsets || !d.consts || d.n_consts <= 0) return remd_fail(h, -1, who + "a CMAP force needs map_index, map_offsets and the maps' blocks in consts");
            for (int k = 0; k < d.n_terms; ++k)
                if (d.map_index[k] < 0 || d.map_index[k] >= d.n_maps) return remd_fail(h, -1, who + "term " + std::to_string(k) + ": map index out of range");
            for (int m = 0; m < d.n_maps; ++m) {
                const std::string map = who + "map " + std::to_string(m) + ": ";
                const long long off = d.map_offsets[m];
                if (off < 0 || off + 8 > (long long)d.n_consts) return remd_fail(h, -1, map + "a block that runs past n_consts");
                const double* B = d.consts + off;
                if (!(B[0] >= 3.0 && B[0] <= 256.0) || B[0] != floor(B[0]) || B[1] != B[0]) return remd_fail(h, -1, map + "a block whose sizes are not nx = ny, an integer 3 ... 256");
                if (B[6] != 1.0) return remd_fail(h, -1, map + "a block that is not periodic");
                if (B[2] != 0.0 || B[4] != 0.0 || !(fabs(B[3] - 2.0 * M_PI) <= 1e-12) || B[5] != B[3]) return remd_fail(h, -1, map + "a block whose range is not [0, 2 pi] in both angles");
                const long long nn = (long long)B[0];
                if (off + 8 + 4 * nn * nn > (long long)d.n_consts) return remd_fail(h, -1, map + "a block that runs past n_consts");
                for (long long k = 0; k < 4 * nn * nn; ++k) if (!std::isfinite(B[8 + k])) return remd_fail(h, -1, map + "a node value that is not finite");
            }
        }
        if (d.n_globals != t.ng) return remd_fail(h, -1, who + "every descriptor must carry the handle's n_globals");
        for (int k = 0; k < t.ng; ++k) if (d.global_defaults && d.global_defaults[k] != t.defaults[k]) return remd_fail(h, -1, who + "global_defaults differ between the descriptors");
        if (d.force_group != desc[0].force_group || d.force_group < 0 || d.force_group > 31)
            return remd_fail(h, -1, who + "every custom force of a handle must sit in one force group (0 ... 31)");
        if (!cmap)       // (a CMAP force has no program)
            if (const char* bad = check_program(d, compound ? 3 * d.n_particles : nonbonded ? 1 : cv ? d.n_cvs : n_vars4[d.kind])) return remd_fail(h, -1, who + bad);
        if (centroid) {
            // the groups: CSR offsets that start at 0 and increase (no empty group), atoms of the system, weights that sum to 1
            if (d.n_groups <= 0 || !d.group_offsets || !d.group_atoms || !d.group_weights) return remd_fail(h, -1, who + "a centroid-bond force needs n_groups > 0, group_offsets, group_atoms and group_weights");
            if (d.group_offsets[0] != 0) return remd_fail(h, -1, who + "group_offsets must start at 0");
            for (int g = 0; g < d.n_groups; ++g) {
                const int b = d.group_offsets[g], e = d.group_offsets[g + 1];
                if (e <= b) return remd_fail(h, -1, who + "group_offsets must increase (an empty group has no centroid)");
                double W = 0.0;
                for (int k = b; k < e; ++k) {
                    if (d.group_atoms[k] < 0 || d.group_atoms[k] >= h->N) return remd_fail(h, -1, who + "group atom index out of range");
                    if (!(d.group_weights[k] >= 0.0)) return remd_fail(h, -1, who + "negative group weight");
                    W += d.group_weights[k];
                }
                if (!(fabs(W - 1.0) <= 1e-12)) return remd_fail(h, -1, who + "the weights of a group must sum to 1 (within 1e-12)");
            }
            for (int k = 0; k < d.n_terms * wd; ++k) if (d.atoms[k] < 0 || d.atoms[k] >= d.n_groups) return remd_fail(h, -1, who + "group index out of range");
        } else
            for (int k = 0; k < d.n_terms * wd; ++k) if (d.atoms[k] < 0 || d.atoms[k] >= h->N) return remd_fail(h, -1, who + "atom index out of range");
        cst_force f{};
        f.kind = d.kind; f.periodic = d.periodic ? 1 : 0; f.n_terms = d.n_terms; f.n_params = d.n_params; f.n_particles = wd;
        f.npad = (d.n_terms + 63) / 64 * 64;
        f.par0 = (int)t.par.size(); f.prog0 = (int)t.prog.size(); f.n_prog = d.n_program; f.const0 = (int)t.consts.size();
        f.switch_dist = -1.0;
        int par_stride = f.npad;
        if (nonbonded) {
            // its wavefronts are the upper-triangular tiles of 64 x 64 atoms; its parameters one row per atom, [n_params][Npad]
            const int nb = (d.n_terms + 63) / 64;
            f.npad = 64 * (nb * (nb + 1) / 2);
            par_stride = h->Npad;
            f.nb_method = d.nb_method; f.cutoff = d.nb_method ? d.cutoff : 0.0; f.switch_dist = d.switch_distance >= 0.0 ? d.switch_distance : -1.0;
            f.lrc = d.long_range_correction ? 1 : 0;
            if (f.lrc) t.has_lrc = true;
            if (d.nb_method == 2) t.periodic_cutoff = std::max(t.periodic_cutoff, d.cutoff);
            f.excl0 = (int)t.excl_off.size();
            const int base = (int)t.excl_atoms.size();
            for (int a = 0; a <= d.n_terms; ++a) t.excl_off.push_back(base + d.excl_offsets[a]);
            if (d.excl_offsets[d.n_terms] > 0) t.excl_atoms.insert(t.excl_atoms.end(), d.excl_atoms, d.excl_atoms + d.excl_offsets[d.n_terms]);
        }
        // parameters [n_params][npad]; a padding slot repeats the last term (finite arithmetic in lanes that add nothing)
        for (int p = 0; p < d.n_params; ++p) for (int s = 0; s < par_stride; ++s) t.par.push_back(d.params[(size_t)std::min(s, d.n_terms - 1) * d.n_params + p]);
        for (int pc = 0; pc < d.n_program; ++pc) t.prog.push_back(make_int2(d.program[2 * pc], d.program[2 * pc + 1]));
        if (d.n_consts > 0) t.consts.insert(t.consts.end(), d.consts, d.consts + d.n_consts);
        if (cv) {
            // its variables join the handle's tables
            f.cv0 = t.n_cv; f.n_cvs = d.n_cvs;
            if (t.cv_off.empty()) t.cv_off.push_back(0);
            const int base = (int)t.cv_atoms.size(), total = d.cv_offsets[d.n_cvs];
            for (int c = 1; c <= d.n_cvs; ++c) t.cv_off.push_back(base + d.cv_offsets[c]);
            t.cv_atoms.insert(t.cv_atoms.end(), d.cv_atoms, d.cv_atoms + total);
            t.cv_ref.insert(t.cv_ref.end(), d.cv_reference, d.cv_reference + 3 * (size_t)total);
            t.n_cv += d.n_cvs;
        }
        if (cmap) {
            // its maps join the handle's: each block's offset in the handle's constants
            f.map0 = (int)t.map_off.size(); f.n_maps = d.n_maps;
            for (int m = 0; m < d.n_maps; ++m) t.map_off.push_back(f.const0 + d.map_offsets[m]);
        }
        t.F.push_back(f);
    }
    // the padded term space: the four one-variable kinds first, the compound-bond forces behind them, then the nonbonded forces' tiles,
    // the centroid-bond forces, the collective-variable forces, the CMAP forces last (each part has its own kernel); the energy columns
    // keep the forces' order whatever their slots
    for (int pass = 0; pass < 6; ++pass) {
        for (int i = 0; i < n; ++i) {
            cst_force& f = t.F[i];
            if ((f.kind == REMD_CUSTOM_CMAP ? 5 : f.kind == REMD_CUSTOM_CV ? 4 : f.kind == REMD_CUSTOM_CENTROID ? 3 : f.kind == REMD_CUSTOM_NONBONDED ? 2 : f.kind == REMD_CUSTOM_COMPOUND ? 1 : 0) != pass) continue;
            f.slot0 = t.total_pad; t.total_pad += f.npad;
            for (int w = 0; w < f.npad / 64; ++w) t.wave_force.push_back(i);
        }
        if (pass == 0) t.waves_simple = t.total_pad / 64;
        if (pass == 1) t.waves_compound = t.total_pad / 64;
        if (pass == 2) t.waves_particles = t.total_pad / 64;
        if (pass == 3) t.waves_centroid = t.total_pad / 64;
        if (pass == 4) t.waves_cv = t.total_pad / 64;
    }
    int rows = 4;
    for (int i = 0; i < n; ++i) rows = std::max(rows, t.F[i].n_particles);
    t.atoms.assign((size_t)rows * t.total_pad, 0);
    // a centroid force's groups join the handle's group tables; its row of `atoms` holds the handle-wide group numbers
    std::vector<int> group0(n, 0);
    for (int i = 0; i < n; ++i) {
        if (t.F[i].kind != REMD_CUSTOM_CENTROID) continue;
        const remd_custom_force_desc& d = desc[i];
        group0[i] = t.n_groups;
        if (t.grp_off.empty()) t.grp_off.push_back(0);
        for (int g = 0; g < d.n_groups; ++g) {
            t.grp_atoms.insert(t.grp_atoms.end(), d.group_atoms + d.group_offsets[g], d.group_atoms + d.group_offsets[g + 1]);
            t.grp_w.insert(t.grp_w.end(), d.group_weights + d.group_offsets[g], d.group_weights + d.group_offsets[g + 1]);
            t.grp_off.push_back((int)t.grp_atoms.size());
            t.grp_periodic.push_back(t.F[i].periodic);
        }
        t.n_groups += d.n_groups;
    }
    for (int i = 0; i < n; ++i) {
        const cst_force& f = t.F[i]; const int wd = f.n_particles;
        for (int s = 0; s < f.npad; ++s) for (int a = 0; a < wd; ++a)
            t.atoms[(size_t)a * t.total_pad + f.slot0 + s] = group0[i] + desc[i].atoms[(size_t)std::min(s, f.n_terms - 1) * wd + a];
    }
    // the map of every slot of the CMAP forces' part (a padding slot repeats the last term's, like its atoms)
    t.map_index.assign((size_t)t.total_pad - (size_t)t.waves_cv * 64, 0);
    for (int i = 0; i < n; ++i) {
        const cst_force& f = t.F[i];
        if (f.kind != REMD_CUSTOM_CMAP) continue;
        for (int s = 0; s < f.npad; ++s) t.map_index[f.slot0 + s - t.waves_cv * 64] = desc[i].map_index[std::min(s, f.n_terms - 1)];
    }
    if (t.n_groups > 0) {
        // per group, every (bond, position) that names it, in table order: the spread kernel adds their gradients in this order
        std::vector<std::vector<int>> named(t.n_groups);
        const int slot_c = t.waves_particles * 64;
        for (int i = 0; i < n; ++i) {
            const cst_force& f = t.F[i];
            if (f.kind != REMD_CUSTOM_CENTROID) continue;
            for (int b = 0; b < f.n_terms; ++b) for (int a = 0; a < f.n_particles; ++a)
                named[t.atoms[(size_t)a * t.total_pad + f.slot0 + b]].push_back((f.slot0 + b - slot_c) * REMD_CUSTOM_MAX_PARTICLES + a);
        }
        t.ref_off.push_back(0);
        for (const std::vector<int>& v : named) { t.refs.insert(t.refs.end(), v.begin(), v.end()); t.ref_off.push_back((int)t.refs.size()); }
    }
    t.K = h->K; t.glob_version = h->states_version; t.uniform = true;
    for (int k = 0; k < std::max(h->K, 0); ++k) t.glob.insert(t.glob.end(), t.defaults.begin(), t.defaults.end());
    if (t.glob.empty()) t.glob.assign(1, 0.0);          // (a force without globals: the kernels still take a pointer)
    t.lrc.assign((size_t)std::max(h->K, 1) * n, 0.0);
    if (t.periodic_cutoff > 0.0 && h->nb_method == REMD_NB_NONE && !h->nocutoff && h->n_bonds + h->n_angles + h->n_torsions + h->n_settle + h->n_shake == 0) {
        // no NonbondedForce and no built-in bonded term or constraint: the molecules a barostat scales are what the custom bonds,
        // angles, torsions and compound bonds join (OpenMM takes molecules from the bonds its forces report); the scaling kernels take
        // contiguous ranges, so a molecule whose atoms are not one gives no table (the barostat then refuses)
        std::vector<int> root(h->N);
        for (int a = 0; a < h->N; ++a) root[a] = a;
        auto find = [&](int a) { while (root[a] != a) a = root[a] = root[root[a]]; return a; };
        for (int i = 0; i < n; ++i) {
            const cst_force& f = t.F[i];
            if (f.kind == REMD_CUSTOM_EXTERNAL || f.kind == REMD_CUSTOM_CENTROID || f.kind == REMD_CUSTOM_NONBONDED || f.kind == REMD_CUSTOM_CV) continue;
            for (int b = 0; b < f.n_terms; ++b) for (int a = 1; a < f.n_particles; ++a) {
                const int p = find(desc[i].atoms[(size_t)b * f.n_particles]), q = find(desc[i].atoms[(size_t)b * f.n_particles + a]);
                if (p != q) root[std::max(p, q)] = std::min(p, q);
            }
        }
        bool contiguous = true;                         // (roots are the lowest atom of a molecule: a range starts at its root)
        for (int a = 0; a < h->N && contiguous; ++a) {
            const int r = find(a);
            if (r == a) { t.mol_first.push_back(a); t.mol_size.push_back(1); }
            else if (r == t.mol_first.back()) t.mol_size.back()++;
            else contiguous = false;
        }
        if (!contiguous) { t.mol_first.clear(); t.mol_size.clear(); }
    }
    remd_custom_release(h);
    h->config_version++;
    int rc = set_tables(h, t);
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
