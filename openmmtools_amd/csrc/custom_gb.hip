// Generalized-Born custom forces (include/remd_hip_custom.h, REMD_CUSTOM_GB): OpenMM's CustomGBForce by its definition -- computed
// values per particle, the first a sum over the other particles, and energy terms per particle and per pair -- with every expression
// a program of the stack machine (custom_machine.h).  The host (openmmtools_amd/custom_gb.py) compiles one program per expression and
// pass: the machine differentiates with respect to three variables, and a stage row says which quantities (r, a value of particle 1
// or 2) they are and which the staged columns are (custom_gb_plan.h lays the rows and the work buffers out).
//
// OpenMM's chain rule in five launches per force, each a grid of one-wavefront workgroups:
//   1  pair value      (row blocks, slices, R): lane i walks the column blocks of its slice, evaluates f(r; i, j) for every j and adds
//                      what counts (j != i, inside the cutoff, not excluded) into a register -> part[slice][i]
//   2  forward         (row blocks, 1, R): V_0 = the slices' sums in slice order; V_1 ... from their programs; the single-particle
//                      energy terms and their dE/dV_k -> V[k][i], dV[k][i]
//   3  pair terms      (row blocks, slices, R): lane i evaluates every term at (min(i, j), max(i, j)) and keeps what belongs to i: half
//                      the energy, the dE/dr force on i, dE/dV_k,i -> dpart[slice][k][i]
//   4  backward        (row blocks, 1, R): dE/dV_k = dV + the slices' sums in slice order; back through V_n-1 ... V_1 -> dV[0][i]
//   5  chain force     (row blocks, slices, R): the force on i is sum_j [dE/dV_0,i df(i,j)/dr + dE/dV_0,j df(j,i)/dr] along x_i - x_j
// A pair is therefore evaluated twice in launch 3 and four times in launch 5; in exchange no lane writes another lane's particle: no
// floating-point atomics, no queue, no order that depends on timing.  The forces leave through the fixed-point accumulators, once per
// lane and launch.  The quantities of a pair come straight from memory: the lane's own at a fixed address (cached), the partner's at a
// wave-uniform one; only the machine's stack and the staged columns live in LDS.  All arithmetic is f64.  r = 0 between distinct
// particles gives an energy and no pair force.  A wavefront skips a column whose 64 pairs all fall away (a wave-uniform branch).
#include "remd_internal.h"
#include "listed_terms.h"
#include "custom_machine.h"

namespace {

struct cgb_args {
    int fi, waves;                          // the force among the handle's; the wavefronts of the whole padded term space
    const cst_force* F; const int* stages; const double* par; const int2* prog; const double* consts;
    const int* excl_off; const int* excl_atoms;
    int Npad; const float4* pos; const float* box; long long* force;
    double* work; size_t work_stride;       // [R][work_stride]
    double* Ewave;                          // [R][waves]
};

struct cgb_ctx {
    cst_force f; cst_gb_work lay; const int* st; const double* par; double* W;
    const float4* P; double Lx, Ly, Lz; bool pbc; double rc2; int N, Npad, nb;
};

__device__ __forceinline__ cgb_ctx cgb_setup(const cgb_args& a, int r)
{
    cgb_ctx c;
    c.f = a.F[a.fi];
    c.lay = cst_gb_layout(a.Npad, c.f.gb_slices, c.f.gb_n_values);
    c.st = a.stages + (size_t)c.f.gb_stage0 * REMD_CUSTOM_GB_STAGE_INTS;
    c.par = a.par + c.f.par0;
    c.W = a.work + (size_t)r * a.work_stride + c.f.gb_work0;
    c.P = a.pos + (size_t)r * a.Npad;
    c.Lx = a.box[4 * r]; c.Ly = a.box[4 * r + 1]; c.Lz = a.box[4 * r + 2];
    c.pbc = c.f.periodic != 0; c.rc2 = c.f.cutoff * c.f.cutoff;
    c.N = c.f.n_terms; c.Npad = a.Npad; c.nb = (c.f.n_terms + 63) / 64;
    return c;
}

// quantity `code` of the pair (p1, p2) (a single particle: p1): r, a value, a parameter; every index lies below Npad
__device__ __forceinline__ double cgb_quantity(const cgb_ctx& c, int code, int p1, int p2, double r)
{
    if (code == 0) return r;
    if (code < 16) return c.W[c.lay.V + (size_t)((code - 1) >> 1) * c.Npad + (((code - 1) & 1) ? p2 : p1)];
    return c.par[(size_t)((code - 16) >> 1) * c.Npad + (((code - 16) & 1) ? p2 : p1)];
}

// stage row g at the pair (p1, p2): the columns staged, the variables loaded, the program run
__device__ __forceinline__ cx cgb_run(const cgb_ctx& c, const int* g, int p1, int p2, double r, const int2* __restrict__ prog,
                                      const double* __restrict__ consts, cst_slot* S, double (*PAR)[64], int lane)
{
    cst_force fl = c.f;
    fl.prog0 = c.f.prog0 + g[CGB_PROG0]; fl.n_prog = g[CGB_NPROG]; fl.par0 = 0; fl.npad = 64;
    for (int k = 0; k < g[CGB_NCOLS]; ++k) PAR[k][lane] = cgb_quantity(c, g[CGB_COL0 + k], p1, p2, r);
    const double x0 = g[CGB_VAR0] >= 0 ? cgb_quantity(c, g[CGB_VAR0], p1, p2, r) : 0.0;
    const double x1 = g[CGB_VAR0 + 1] >= 0 ? cgb_quantity(c, g[CGB_VAR0 + 1], p1, p2, r) : 0.0;
    const double x2 = g[CGB_VAR0 + 2] >= 0 ? cgb_quantity(c, g[CGB_VAR0 + 2], p1, p2, r) : 0.0;
    return cst_eval<false>(fl, prog, consts, &PAR[0][0], lane, nullptr, x0, x1, x2, c.Lx, c.Ly, c.Lz, S, lane);
}

__device__ __forceinline__ double cgb_partial(const cx& e, int v) { return v == 0 ? e.a : v == 1 ? e.b : e.c; }

// the lane's exclusion row folded into a mask of column block jb
__device__ __forceinline__ unsigned long long cgb_excluded(const cgb_ctx& c, const int* __restrict__ excl_off, const int* __restrict__ excl_atoms, int i, int jb)
{
    unsigned long long ex = 0ull;
    if (i < c.N)
        for (int k = excl_off[c.f.excl0 + i]; k < excl_off[c.f.excl0 + i + 1]; ++k) {
            const int d = excl_atoms[k] - jb * 64;
            if (d >= 0 && d < 64) ex |= 1ull << d;
        }
    return ex;
}

struct cgb_pair { bool near; double r, ux, uy, uz; };     // near: two distinct real particles inside the cutoff; u = (x_j - x_i) / r, 0 at r = 0

__device__ __forceinline__ cgb_pair cgb_geometry(const cgb_ctx& c, const float4& pi, int i, int j)
{
    cgb_pair p;
    const double3 d = d3img(d3sub(c.P[j], pi), c.pbc, c.Lx, c.Ly, c.Lz);
    const double r2 = d3dot(d, d);
    p.r = sqrt(r2);
    const double ir = p.r > 0.0 ? 1.0 / p.r : 0.0;
    p.ux = d.x * ir; p.uy = d.y * ir; p.uz = d.z * ir;
    p.near = i < c.N && j < c.N && i != j && (c.f.nb_method == 0 || r2 < c.rc2);
    return p;
}

// launch 1: part[slice][i] = sum over the slice's j of f(r; i, j)
__global__ __launch_bounds__(64)
void custom_gb_value_kernel(cgb_args a)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    const int lane = threadIdx.x, s = blockIdx.y, r = blockIdx.z, i = blockIdx.x * 64 + lane;
    const cgb_ctx c = cgb_setup(a, r);
    const int* g = c.st;                                       // (stage 0)
    const float4 pi = c.P[i];
    double acc = 0.0;
    for (int jb = cst_gb_slice_begin(c.nb, c.f.gb_slices, s); jb < cst_gb_slice_begin(c.nb, c.f.gb_slices, s + 1); ++jb) {
        const unsigned long long ex = g[CGB_EXCL] ? cgb_excluded(c, a.excl_off, a.excl_atoms, i, jb) : 0ull;
        for (int jj = 0; jj < 64; ++jj) {
            const int j = jb * 64 + jj;
            const cgb_pair p = cgb_geometry(c, pi, i, j);
            const bool on = p.near && !((ex >> jj) & 1ull);
            if (__ballot(on) == 0ull) continue;
            const cx e = cgb_run(c, g, i, j, p.r, a.prog, a.consts, S, PAR, lane);
            acc += on ? e.v : 0.0;
        }
    }
    c.W[c.lay.part + (size_t)s * c.Npad + i] = acc;
}

// launch 2: the values, the single-particle terms and their dE/dV_k
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_gb_forward_kernel(cgb_args a)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ double G[REMD_CUSTOM_GB_MAX_VALUES][64];
    const int lane = threadIdx.x, r = blockIdx.z, i = blockIdx.x * 64 + lane;
    const cgb_ctx c = cgb_setup(a, r);
    double v0 = 0.0;
    for (int s = 0; s < c.f.gb_slices; ++s) v0 += c.W[c.lay.part + (size_t)s * c.Npad + i];
    c.W[c.lay.V + i] = v0;
    for (int k = 0; k < REMD_CUSTOM_GB_MAX_VALUES; ++k) G[k][lane] = 0.0;
    double E = 0.0;
    for (int q = 1; q < c.f.gb_n_stages; ++q) {
        const int* g = c.st + (size_t)q * REMD_CUSTOM_GB_STAGE_INTS;
        if (g[CGB_TYPE] == CGB_SINGLE_VALUE) {
            // (the lane reads back what it stored itself: values of its own particle only)
            const cx e = cgb_run(c, g, i, i, 0.0, a.prog, a.consts, S, PAR, lane);
            c.W[c.lay.V + (size_t)g[CGB_TARGET] * c.Npad + i] = e.v;
        } else if (g[CGB_TYPE] == CGB_SINGLE_ENERGY) {
            const cx e = cgb_run(c, g, i, i, 0.0, a.prog, a.consts, S, PAR, lane);
            if (g[CGB_PASS] == 0) E += e.v;
            for (int v = 0; v < 3; ++v) if (g[CGB_VAR0 + v] >= 1) G[(g[CGB_VAR0 + v] - 1) >> 1][lane] += cgb_partial(e, v);
        }
    }
    for (int k = 0; k < c.f.gb_n_values; ++k) c.W[c.lay.dV + (size_t)k * c.Npad + i] = G[k][lane];
    if (ENERGY) {
        const double ew = cst_wave_sum(i < c.N ? E : 0.0);
        if (lane == 0) a.Ewave[(size_t)r * a.waves + c.f.slot0 / 64 + c.nb * c.f.gb_slices + blockIdx.x] = ew;
    }
}

// launch 3: the pair terms, lane i keeping what belongs to particle i
template <bool ENERGY>
__global__ __launch_bounds__(64)
void custom_gb_pair_kernel(cgb_args a)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ double G[REMD_CUSTOM_GB_MAX_VALUES][64];
    const int lane = threadIdx.x, s = blockIdx.y, r = blockIdx.z, i = blockIdx.x * 64 + lane;
    const cgb_ctx c = cgb_setup(a, r);
    for (int k = 0; k < REMD_CUSTOM_GB_MAX_VALUES; ++k) G[k][lane] = 0.0;
    int first = c.f.gb_n_stages;                               // the first pair term among the stages (none: nothing to walk)
    for (int q = c.f.gb_n_stages - 1; q >= 1; --q) if (c.st[(size_t)q * REMD_CUSTOM_GB_STAGE_INTS + CGB_TYPE] == CGB_PAIR_ENERGY) first = q;
    const float4 pi = c.P[i];
    double E = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
    if (first < c.f.gb_n_stages)
        for (int jb = cst_gb_slice_begin(c.nb, c.f.gb_slices, s); jb < cst_gb_slice_begin(c.nb, c.f.gb_slices, s + 1); ++jb) {
            const unsigned long long ex = cgb_excluded(c, a.excl_off, a.excl_atoms, i, jb);
            for (int jj = 0; jj < 64; ++jj) {
                const int j = jb * 64 + jj;
                const cgb_pair p = cgb_geometry(c, pi, i, j);
                if (__ballot(p.near) == 0ull) continue;
                const bool lower = i < j;                      // particle 1 is the lower index; own: which of the two is i
                const int p1 = lower ? i : j, p2 = lower ? j : i, own = lower ? 0 : 1;
                for (int q = first; q < c.f.gb_n_stages; ++q) {
                    const int* g = c.st + (size_t)q * REMD_CUSTOM_GB_STAGE_INTS;
                    if (g[CGB_TYPE] != CGB_PAIR_ENERGY) continue;
                    const bool on = p.near && !(g[CGB_EXCL] && ((ex >> jj) & 1ull));
                    if (__ballot(on) == 0ull) continue;
                    const cx e = cgb_run(c, g, p1, p2, p.r, a.prog, a.consts, S, PAR, lane);
                    if (!on) continue;
                    if (g[CGB_PASS] == 0) E += 0.5 * e.v;
                    for (int v = 0; v < 3; ++v) {
                        const int code = g[CGB_VAR0 + v];
                        const double d = cgb_partial(e, v);
                        if (code == 0) { fx += d * p.ux; fy += d * p.uy; fz += d * p.uz; }      // the force on i is +dE/dr (x_j - x_i) / r
                        else if (code > 0 && ((code - 1) & 1) == own) G[(code - 1) >> 1][lane] += d;
                    }
                }
            }
        }
    for (int k = 0; k < c.f.gb_n_values; ++k) c.W[c.lay.dpart + ((size_t)s * c.f.gb_n_values + k) * c.Npad + i] = G[k][lane];
    if (i < c.N && first < c.f.gb_n_stages) add_force(a.force + (size_t)r * 3 * a.Npad, a.Npad, i, (float)fx, (float)fy, (float)fz);
    if (ENERGY) {
        const double ew = cst_wave_sum(i < c.N ? E : 0.0);
        if (lane == 0) a.Ewave[(size_t)r * a.waves + c.f.slot0 / 64 + blockIdx.x * c.f.gb_slices + s] = ew;
    }
}

// launch 4: dE/dV_k summed in a fixed order, then back through the single-particle values to dE/dV_0
__global__ __launch_bounds__(64)
void custom_gb_backward_kernel(cgb_args a)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    __shared__ double G[REMD_CUSTOM_GB_MAX_VALUES][64];
    const int lane = threadIdx.x, r = blockIdx.z, i = blockIdx.x * 64 + lane;
    const cgb_ctx c = cgb_setup(a, r);
    for (int k = 0; k < REMD_CUSTOM_GB_MAX_VALUES; ++k) G[k][lane] = 0.0;
    for (int k = 0; k < c.f.gb_n_values; ++k) {
        double d = c.W[c.lay.dV + (size_t)k * c.Npad + i];
        for (int s = 0; s < c.f.gb_slices; ++s) d += c.W[c.lay.dpart + ((size_t)s * c.f.gb_n_values + k) * c.Npad + i];
        G[k][lane] = d;
    }
    for (int q = c.f.gb_n_values - 1; q >= 1; --q) {           // (stage q is value q: the values come first, in order)
        const int* g = c.st + (size_t)q * REMD_CUSTOM_GB_STAGE_INTS;
        const cx e = cgb_run(c, g, i, i, 0.0, a.prog, a.consts, S, PAR, lane);
        const double up = G[q][lane];
        for (int v = 0; v < 3; ++v) if (g[CGB_VAR0 + v] >= 1) G[(g[CGB_VAR0 + v] - 1) >> 1][lane] += up * cgb_partial(e, v);
    }
    c.W[c.lay.dV + i] = G[0][lane];
}

// launch 5: the force of the pair value's dependence on r, both directions
__global__ __launch_bounds__(64)
void custom_gb_chain_kernel(cgb_args a)
{
    __shared__ cst_slot S[REMD_CUSTOM_MAX_STACK];
    __shared__ double PAR[REMD_CUSTOM_MAX_PARAMS][64];
    const int lane = threadIdx.x, s = blockIdx.y, r = blockIdx.z, i = blockIdx.x * 64 + lane;
    const cgb_ctx c = cgb_setup(a, r);
    const int* g = c.st;
    const float4 pi = c.P[i];
    const double gi = c.W[c.lay.dV + i];
    double fx = 0.0, fy = 0.0, fz = 0.0;
    for (int jb = cst_gb_slice_begin(c.nb, c.f.gb_slices, s); jb < cst_gb_slice_begin(c.nb, c.f.gb_slices, s + 1); ++jb) {
        const unsigned long long ex = g[CGB_EXCL] ? cgb_excluded(c, a.excl_off, a.excl_atoms, i, jb) : 0ull;
        for (int jj = 0; jj < 64; ++jj) {
            const int j = jb * 64 + jj;
            const cgb_pair p = cgb_geometry(c, pi, i, j);
            const bool on = p.near && !((ex >> jj) & 1ull);
            if (__ballot(on) == 0ull) continue;
            const double dij = cgb_run(c, g, i, j, p.r, a.prog, a.consts, S, PAR, lane).a;
            const double dji = cgb_run(c, g, j, i, p.r, a.prog, a.consts, S, PAR, lane).a;
            if (!on) continue;
            const double k = gi * dij + c.W[c.lay.dV + j] * dji;       // dE/dr of the pair through both particles' values
            fx += k * p.ux; fy += k * p.uy; fz += k * p.uz;
        }
    }
    if (i < c.N) add_force(a.force + (size_t)r * 3 * a.Npad, a.Npad, i, (float)fx, (float)fy, (float)fz);
}

}  // namespace

void remd_custom_gb_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st)
{
    for (int fi = 0; fi < t.nf; ++fi) {
        const cst_force& f = t.F[fi];
        if (f.kind != REMD_CUSTOM_GB) continue;
        const int nb = (f.n_terms + 63) / 64;
        const cgb_args a{fi, t.total_pad / 64, t.d_F, t.d_gb_stages, t.d_par, t.d_prog, t.d_consts, t.d_excl_off, t.d_excl_atoms,
                         h->Npad, h->d_pos, h->d_box, h->d_force, t.d_gb_work, t.gb_work, t.d_Ewave};
        const dim3 pairs(nb, f.gb_slices, h->R), particles(nb, 1, h->R);
        hipLaunchKernelGGL(custom_gb_value_kernel, pairs, dim3(64), 0, st, a);
        if (with_energy) hipLaunchKernelGGL(custom_gb_forward_kernel<true>, particles, dim3(64), 0, st, a);
        else hipLaunchKernelGGL(custom_gb_forward_kernel<false>, particles, dim3(64), 0, st, a);
        if (with_energy) hipLaunchKernelGGL(custom_gb_pair_kernel<true>, pairs, dim3(64), 0, st, a);
        else hipLaunchKernelGGL(custom_gb_pair_kernel<false>, pairs, dim3(64), 0, st, a);
        hipLaunchKernelGGL(custom_gb_backward_kernel, particles, dim3(64), 0, st, a);
        hipLaunchKernelGGL(custom_gb_chain_kernel, pairs, dim3(64), 0, st, a);
    }
}
