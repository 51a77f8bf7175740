// The stack machine of the custom forces (include/remd_hip_custom.h), shared by custom_terms.hip (bond, angle, torsion, external),
// custom_compound.hip (compound bonds), custom_centroid.hip (centroid bonds, whose particles are centroids), custom_cv.hip
// (collective variables, whose variables are RMSDs), custom_hbond.hip (donor-acceptor pairs, whose particles are d1 d2 d3 a1 a2 a3) and
// custom_manyparticle.hip (sets of three particles p1 p2 p3): the handle's tables (the per-force record and the host plan behind them live in
// custom_plan.h, which needs no HIP) and cst_eval, which runs a postfix program one term per lane with every stack slot a value and three partials, the stack in LDS as [slot][component][lane].
// cmap.hip (CMAP torsion maps) runs no program: it shares the record, the tables and the patch of two arguments (table2d_patch.h).
//
// cst_eval<GEOM>: the instantiation of the four one-variable kinds (GEOM = false) has the variables in three registers and no case
// for the opcodes of particles; the one of a compound-bond force (GEOM = true) reads the variables x1 y1 z1 ... from the lane's
// particle positions in LDS, [particle][component][lane], and knows REMD_CX_DISTANCE / ANGLE / DIHEDRAL.  Its partials are the
// gradient with respect to ONE particle, `seed`: the coordinates of that particle carry the unit partials, every other coordinate
// carries zero, and an opcode of particles pushes its value with its gradient with respect to particle `seed` (zero where `seed` is
// not among its arguments; formulas and guards of cst_geometry in custom_terms.hip).  seed = -1: values only.
// Both instantiations know the tabulated functions, REMD_CX_TABLE1D / REMD_CX_LOOKUP1D (cst_table1d, cst_lookup1d below) and
// REMD_CX_TABLE2D / REMD_CX_LOOKUP2D / REMD_CX_LOOKUP3D (cst_table2d, cst_lookup2d, cst_lookup3d).
#pragma once
#include "remd_internal.h"
#include "custom_plan.h"
#include "table2d_patch.h"

// what a handle with custom forces owns: the plan of the set-up (custom_plan.h: every host table, the scalars and the parts of the
// padded term space), its tables on the device under the same names with d_ in front, and the work buffers of the launches
struct cst_tables : cst_plan {
    dev_array<cst_force> d_F; dev_array<int> d_wave_force, d_atoms; dev_array<double> d_par, d_consts, d_glob; dev_array<int2> d_prog;
    dev_array<int> d_grp_off, d_grp_atoms, d_grp_periodic, d_ref_off, d_refs; dev_array<double> d_grp_w;
    dev_array<int> d_cv_off, d_cv_atoms; dev_array<double> d_cv_ref;
    dev_array<int> d_map_off, d_map_index;
    dev_array<int> d_hb_atoms;
    dev_array<int> d_mp_types;
    dev_array<int> d_excl_off, d_excl_atoms; dev_array<double> d_lrc;
    dev_array<int> d_mol_first, d_mol_size;
    dev_array<double> d_E;             // [R][nf]
    dev_array<double> d_Ewave;         // [R][total_pad / 64]
    dev_array<double> d_D;             // [R][K][total_pad / 64] u_kl partials
    dev_array<int> d_dcols; dev_array<unsigned> d_dmask;   // the declared energy parameter derivatives (cst_plan::dcols, dmask); empty: none
    dev_array<double> d_dD;            // [R][n_derivatives][total_pad / 64] their partials; allocated by the first remd_get_custom_parameter_derivatives
    dev_array<double> d_dOut;          // [R][n_derivatives] dE/dglobal
    dev_array<double> d_dDK;           // [R][K][n_derivatives][total_pad / 64] the same under every state's globals; allocated by the first
    dev_array<double> d_dOutK;         // [R][K][n_derivatives]                 remd_get_custom_parameter_derivatives_at_states
    dev_array<double> d_C;             // [R][n_groups][3] centroids
    dev_array<double> d_G;             // [R][centroid slots][REMD_CUSTOM_MAX_PARTICLES][3] dE / d centroid
    dev_array<double> d_W;             // [R][n_cv][16]: RMSD, "no force" flag, centroid, rotation, dE/dRMSD (custom_cv.hip)
    dev_array<int> d_mp_nbr;           // [R][mp_rows][REMD_CUSTOM_MP_MAX_NEIGHBORS]: the neighbour rows of the many-particle forces (custom_manyparticle.hip)
    dev_array<int> d_mp_cnt;           // [R][mp_rows]: their counts (which may exceed a row: the row then holds its first entries)
    dev_array<int> d_gb_stages;        // the stage rows of the Generalized-Born forces (custom_gb.hip)
    dev_array<double> d_gb_work;       // [R][gb_work]: their partial sums, values and dE/dV (custom_gb_plan.h)
};

namespace {

struct cx { double v, a, b, c; };       // a value and its partials
typedef double cst_slot[4][64];

__device__ __forceinline__ cx cx_ld(const cst_slot* S, int sp, int lane) { return cx{S[sp][0][lane], S[sp][1][lane], S[sp][2][lane], S[sp][3][lane]}; }
__device__ __forceinline__ void cx_st(cst_slot* S, int sp, int lane, const cx& x) { S[sp][0][lane] = x.v; S[sp][1][lane] = x.a; S[sp][2][lane] = x.b; S[sp][3][lane] = x.c; }
__device__ __forceinline__ cx cx_chain(double v, double k, const cx& x) { return cx{v, k * x.a, k * x.b, k * x.c}; }

__device__ __forceinline__ double cst_image(double d, double L) { return L > 0.0 ? d - L * rint(d / L) : d; }

// a ^ n by multiplications (n >= 0)
__device__ __forceinline__ double cst_ipow(double a, int n)
{
    double r = 1.0;
    for (; n > 0; n >>= 1) { if (n & 1) r *= a; a *= a; }
    return r;
}

__device__ __forceinline__ double3 d3(double x, double y, double z) { return make_double3(x, y, z); }
__device__ __forceinline__ double3 d3sub(const float4& a, const float4& b) { return d3((double)a.x - (double)b.x, (double)a.y - (double)b.y, (double)a.z - (double)b.z); }
__device__ __forceinline__ double3 d3sub(double3 a, double3 b) { return d3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ double d3dot(double3 a, double3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double3 d3crs(double3 a, double3 b) { return d3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ double3 d3scl(double3 a, double s) { return d3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ double3 d3add(double3 a, double3 b) { return d3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ double3 d3img(double3 d, bool pbc, double Lx, double Ly, double Lz)
{
    return pbc ? d3(cst_image(d.x, Lx), cst_image(d.y, Ly), cst_image(d.z, Lz)) : d;
}

typedef double cst_pos[3][64];          // one particle of a compound bond: [component][lane]

__device__ __forceinline__ double3 cst_ldpos(const cst_pos* X, int q, int lane) { return d3(X[q][0][lane], X[q][1][lane], X[q][2][lane]); }
__device__ __forceinline__ double3 d3pick(bool on, double3 a) { return d3(on ? a.x : 0.0, on ? a.y : 0.0, on ? a.z : 0.0); }

// distance / angle / dihedral of the particle slots packed in `arg`, with the gradient with respect to particle `seed`; differences
// are minimum images where the box lengths are positive (the caller passes 0 for a force that is not periodic)
__device__ __forceinline__ cx cst_particles_op(int op, int arg, int seed, const cst_pos* X, int lane, double Lx, double Ly, double Lz)
{
    const int s0 = arg & 15, s1 = (arg >> 4) & 15;
    const double3 p0 = cst_ldpos(X, s0, lane), p1 = cst_ldpos(X, s1, lane);
    double v; double3 g;
    if (op == REMD_CX_DISTANCE) {
        const double3 d = d3img(d3sub(p1, p0), true, Lx, Ly, Lz);
        const double r = sqrt(d3dot(d, d)), ir = r > 0.0 ? 1.0 / r : 0.0;
        v = r;
        g = d3add(d3pick(s1 == seed, d3scl(d, ir)), d3pick(s0 == seed, d3scl(d, -ir)));
    } else if (op == REMD_CX_ANGLE) {
        const int s2 = (arg >> 8) & 15;
        const double3 p2 = cst_ldpos(X, s2, lane);
        const double3 v0 = d3img(d3sub(p0, p1), true, Lx, Ly, Lz), v1 = d3img(d3sub(p2, p1), true, Lx, Ly, Lz);
        const double3 cp = d3crs(v0, v1);
        const double rp = fmax(sqrt(d3dot(cp, cp)), 1e-6);
        const double r20 = d3dot(v0, v0), r21 = d3dot(v1, v1);
        v = acos(fmin(fmax(d3dot(v0, v1) / sqrt(r20 * r21), -1.0), 1.0));
        const double3 g0 = d3scl(d3crs(v0, cp), 1.0 / (r20 * rp)), g2 = d3scl(d3crs(cp, v1), 1.0 / (r21 * rp));
        const double3 g1 = d3scl(d3add(g0, g2), -1.0);
        g = d3add(d3add(d3pick(s0 == seed, g0), d3pick(s1 == seed, g1)), d3pick(s2 == seed, g2));
    } else {
        const int s2 = (arg >> 8) & 15, s3 = (arg >> 12) & 15;
        const double3 p2 = cst_ldpos(X, s2, lane), p3 = cst_ldpos(X, s3, lane);
        const double3 b1 = d3img(d3sub(p1, p0), true, Lx, Ly, Lz), b2 = d3img(d3sub(p2, p1), true, Lx, Ly, Lz);
        const double3 b3 = d3img(d3sub(p3, p2), true, Lx, Ly, Lz);
        const double3 m = d3crs(b1, b2), nn = d3crs(b2, b3);
        const double m2 = fmax(d3dot(m, m), 1e-24), n2 = fmax(d3dot(nn, nn), 1e-24);
        const double lb2 = sqrt(d3dot(b2, b2));
        v = atan2(lb2 * d3dot(b1, nn), d3dot(m, nn));
        const double3 g0 = d3scl(m, -lb2 / m2), g3 = d3scl(nn, lb2 / n2);
        const double s12 = d3dot(b1, b2) / (lb2 * lb2), s32 = d3dot(b3, b2) / (lb2 * lb2);
        const double3 g1 = d3add(d3scl(g0, -(1.0 + s12)), d3scl(g3, s32)), g2 = d3add(d3scl(g3, -(1.0 + s32)), d3scl(g0, s12));
        g = d3add(d3add(d3pick(s0 == seed, g0), d3pick(s1 == seed, g1)), d3add(d3pick(s2 == seed, g2), d3pick(s3 == seed, g3)));
    }
    return cx{v, g.x, g.y, g.z};
}

// Tabulated functions (include/remd_hip_custom.h: REMD_CX_TABLE1D, REMD_CX_LOOKUP1D).  B is the function's block in the force's
// constants, consts + f.const0 + operand: wave-uniform, so the header loads are; the loads of y and y'' are one gather per lane.
// remd_set_custom_terms has checked the header and that the block ends inside the constants (check_program), so an index is safe
// exactly when it lies inside the block.  That must hold for EVERY argument: the padding lanes of a wavefront, and of a nonbonded
// tile, run the program on whatever their registers hold (a repeated last term, a distance of atoms that are not a pair, possibly
// huge, infinite or NaN), and a function of a variable is handed whatever the geometry gives.  Hence: the argument is range-tested
// in f64 first (a NaN fails every comparison), only a value that passed is converted to an integer, the integer is clamped again,
// and a lane that failed loads nothing.  Such a lane pushes 0 (OpenMM's value outside the range), or NaN for a NaN.
__device__ __forceinline__ void cst_table1d(const double* __restrict__ B, double x, double& v, double& k)
{
    const int n = (int)B[0];                                  // 2 ... REMD_CUSTOM_MAX_TABLE_POINTS
    const double lo = B[1], hi = B[2], L = hi - lo, h = L / (double)(n - 1);
    // periodic: into [min, max); the rounding of the wrap may leave it an ulp outside, so it is clamped (an argument too large to
    // have a place in the period lands on an end; an infinite one gives NaN, which the comparisons keep: fmin / fmax would drop it)
    const double w = x - L * floor((x - lo) / L);
    const double t = B[3] != 0.0 ? (w < lo ? lo : w > hi ? hi : w) : x;
    const bool inside = t >= lo && t <= hi;
    const double s = inside ? (t - lo) / h : 0.0;                            // in [0, n - 1] (rounding aside) where it is converted
    const int i = min(max((int)s, 0), n - 2);
    v = t != t ? t : 0.0; k = 0.0;
    if (inside) {
        const double y0 = B[4 + i], y1 = B[5 + i], d0 = B[4 + n + i], d1 = B[5 + n + i];
        const double b = s - (double)i, a = 1.0 - b;          // (t - x_i) / h; a = (x_{i+1} - t) / h as 1 - b, so that a + b is exactly 1
        v = a * y0 + b * y1 + ((a * a * a - a) * d0 + (b * b * b - b) * d1) * (h * h / 6.0);
        k = (y1 - y0) / h + ((1.0 - 3.0 * a * a) * d0 + (3.0 * b * b - 1.0) * d1) * (h / 6.0);
    }
}

// values[round(x)], halves away from zero; NaN, and no load, where the index falls outside 0 ... n - 1 (the device cannot raise)
__device__ __forceinline__ double cst_lookup1d(const double* __restrict__ B, double x)
{
    const double r = round(x), last = B[0] - 1.0;            // B[0] = n, 1 ... REMD_CUSTOM_MAX_TABLE_POINTS
    const bool inside = r >= 0.0 && r <= last;
    const int i = inside ? (int)r : 0;
    double v = __builtin_nan("");
    if (inside) v = B[1 + i];
    return v;
}

// cst_table_axis and cst_table2d, the bicubic Hermite patch of REMD_CX_TABLE2D, live in table2d_patch.h: cmap.hip evaluates the same patch.

// values[round(x) + nx round(y)] of the block [nx, ny], values[ny][nx]; NaN, and no load, where an index falls outside its range
__device__ __forceinline__ double cst_lookup2d(const double* __restrict__ B, double x, double y)
{
    const double rx = round(x), ry = round(y);
    const int nx = (int)B[0], ny = (int)B[1];                // >= 1, nx ny <= REMD_CUSTOM_MAX_TABLE_CELLS
    const bool inside = rx >= 0.0 && rx <= (double)(nx - 1) && ry >= 0.0 && ry <= (double)(ny - 1);
    const int i = inside ? min(max((int)rx, 0), nx - 1) : 0, j = inside ? min(max((int)ry, 0), ny - 1) : 0;
    double v = __builtin_nan("");
    if (inside) v = B[2 + j * nx + i];
    return v;
}

// values[round(x) + nx round(y) + nx ny round(z)] of the block [nx, ny, nz, 0], values[nz][ny][nx]
__device__ __forceinline__ double cst_lookup3d(const double* __restrict__ B, double x, double y, double z)
{
    const double rx = round(x), ry = round(y), rz = round(z);
    const int nx = (int)B[0], ny = (int)B[1], nz = (int)B[2];
    const bool inside = rx >= 0.0 && rx <= (double)(nx - 1) && ry >= 0.0 && ry <= (double)(ny - 1) && rz >= 0.0 && rz <= (double)(nz - 1);
    const int i = inside ? min(max((int)rx, 0), nx - 1) : 0, j = inside ? min(max((int)ry, 0), ny - 1) : 0;
    const int k = inside ? min(max((int)rz, 0), nz - 1) : 0;
    double v = __builtin_nan("");
    if (inside) v = B[4 + (k * ny + j) * nx + i];
    return v;
}

// the program of force f at term t (lane's own) under the globals g (wave-uniform); the result's partials are dE/dvariable
// (GEOM: dE/d(x, y, z) of particle `seed`; x0, x1, x2 are not read)
// DPAR (energy parameter derivatives, remd_get_custom_parameter_derivatives): the differentiated quantity is global column `dcol`
// instead of the variables -- that REMD_CX_GLOBAL push carries the unit partial in component a, every variable is pushed with zero
// partials (GEOM: the caller passes seed = -1, so coordinates and functions of particles are), and the result's a is dE/dglobal.
// A compile-time switch: the instantiations without it are the code they were.
template <bool GEOM, bool DPAR = false>
__device__ __forceinline__ cx cst_eval(const cst_force& f, const int2* __restrict__ prog, const double* __restrict__ consts,
                                       const double* __restrict__ par, int t, const double* __restrict__ g, double x0, double x1,
                                       double x2, double Lx, double Ly, double Lz, cst_slot* S, int lane,
                                       const cst_pos* X = nullptr, int seed = -1, int dcol = -1)
{
    int sp = 0;
    for (int pc = 0; pc < f.n_prog; ++pc) {
        const int2 ins = prog[f.prog0 + pc];
        const int op = ins.x, arg = ins.y;
        switch (op) {
        case REMD_CX_CONST:  cx_st(S, sp++, lane, cx{consts[f.const0 + arg], 0.0, 0.0, 0.0}); break;
        // (variable `arg` has the unit partial `arg`; scalars picked by value: a pick among structs becomes a pick of addresses in scratch)
        case REMD_CX_VAR:
            if (GEOM) {
                const int q = arg / 3, c = arg - 3 * q;
                const bool on = q == seed;
                cx_st(S, sp++, lane, cx{X[q][c][lane], on && c == 0 ? 1.0 : 0.0, on && c == 1 ? 1.0 : 0.0, on && c == 2 ? 1.0 : 0.0});
            } else if (DPAR)
                cx_st(S, sp++, lane, cx{arg == 0 ? x0 : arg == 1 ? x1 : x2, 0.0, 0.0, 0.0});
            else
                cx_st(S, sp++, lane, cx{arg == 0 ? x0 : arg == 1 ? x1 : x2, arg == 0 ? 1.0 : 0.0, arg == 1 ? 1.0 : 0.0, arg == 2 ? 1.0 : 0.0});
            break;
        case REMD_CX_PARAM:  cx_st(S, sp++, lane, cx{par[f.par0 + (size_t)arg * f.npad + t], 0.0, 0.0, 0.0}); break;
        case REMD_CX_GLOBAL: cx_st(S, sp++, lane, cx{g[arg], DPAR && arg == dcol ? 1.0 : 0.0, 0.0, 0.0}); break;
        case REMD_CX_ADD: case REMD_CX_SUB: case REMD_CX_MUL: case REMD_CX_DIV: case REMD_CX_POW: case REMD_CX_ATAN2:
        case REMD_CX_MIN: case REMD_CX_MAX: case REMD_CX_TABLE2D: case REMD_CX_LOOKUP2D: {
            const cx x = cx_ld(S, sp - 2, lane), y = cx_ld(S, sp - 1, lane);
            cx z;
            if (op == REMD_CX_ADD) z = cx{x.v + y.v, x.a + y.a, x.b + y.b, x.c + y.c};
            else if (op == REMD_CX_SUB) z = cx{x.v - y.v, x.a - y.a, x.b - y.b, x.c - y.c};
            else if (op == REMD_CX_MUL) z = cx{x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b, x.c * y.v + x.v * y.c};
            else if (op == REMD_CX_DIV) {
                const double q = x.v / y.v, iy = 1.0 / y.v;
                z = cx{q, (x.a - q * y.a) * iy, (x.b - q * y.b) * iy, (x.c - q * y.c) * iy};
            } else if (op == REMD_CX_POW) {
                // d(x^y) = y x^(y-1) dx + x^y ln x dy; the second term only where the exponent varies (ln of a base <= 0 otherwise
                // poisons a constant exponent's zero partial)
                const double p = pow(x.v, y.v), kx = y.v * pow(x.v, y.v - 1.0);
                const bool yvar = y.a != 0.0 || y.b != 0.0 || y.c != 0.0;
                const double ky = yvar ? p * log(x.v) : 0.0;
                z = cx{p, kx * x.a + ky * y.a, kx * x.b + ky * y.b, kx * x.c + ky * y.c};
            } else if (op == REMD_CX_ATAN2) {
                const double n2 = 1.0 / (x.v * x.v + y.v * y.v);          // atan2(x, y): x the sine-like argument
                z = cx{atan2(x.v, y.v), (y.v * x.a - x.v * y.a) * n2, (y.v * x.b - x.v * y.b) * n2, (y.v * x.c - x.v * y.c) * n2};
            } else if (op == REMD_CX_TABLE2D) {
                double v, kx, ky;
                cst_table2d(consts + f.const0 + arg, x.v, y.v, v, kx, ky);
                z = cx{v, kx * x.a + ky * y.a, kx * x.b + ky * y.b, kx * x.c + ky * y.c};
            } else if (op == REMD_CX_LOOKUP2D) z = cx{cst_lookup2d(consts + f.const0 + arg, x.v, y.v), 0.0, 0.0, 0.0};
            else if (op == REMD_CX_MIN) z = x.v < y.v ? x : y;
            else z = x.v > y.v ? x : y;
            cx_st(S, sp - 2, lane, z); --sp;
        } break;
        case REMD_CX_SELECT: {
            const cx x = cx_ld(S, sp - 3, lane), y = cx_ld(S, sp - 2, lane), z = cx_ld(S, sp - 1, lane);
            cx_st(S, sp - 3, lane, x.v != 0.0 ? y : z); sp -= 2;
        } break;
        case REMD_CX_LOOKUP3D:                            // the arguments' values only: the result's partials are zero
            cx_st(S, sp - 3, lane, cx{cst_lookup3d(consts + f.const0 + arg, S[sp - 3][0][lane], S[sp - 2][0][lane], S[sp - 1][0][lane]), 0.0, 0.0, 0.0});
            sp -= 2;
            break;
        case REMD_CX_PERIODICDISTANCE: {
            const cx x1 = cx_ld(S, sp - 6, lane), y1 = cx_ld(S, sp - 5, lane), z1 = cx_ld(S, sp - 4, lane);
            const cx x2 = cx_ld(S, sp - 3, lane), y2 = cx_ld(S, sp - 2, lane), z2 = cx_ld(S, sp - 1, lane);
            const double dx = cst_image(x2.v - x1.v, Lx), dy = cst_image(y2.v - y1.v, Ly), dz = cst_image(z2.v - z1.v, Lz);
            const double d = sqrt(dx * dx + dy * dy + dz * dz), id = d > 0.0 ? 1.0 / d : 0.0;
            const double ux = dx * id, uy = dy * id, uz = dz * id;
            cx_st(S, sp - 6, lane, cx{d, ux * (x2.a - x1.a) + uy * (y2.a - y1.a) + uz * (z2.a - z1.a),
                                         ux * (x2.b - x1.b) + uy * (y2.b - y1.b) + uz * (z2.b - z1.b),
                                         ux * (x2.c - x1.c) + uy * (y2.c - y1.c) + uz * (z2.c - z1.c)});
            sp -= 5;
        } break;
        default: {                                        // one argument, or (GEOM) a function of particles: no argument
            if (GEOM && op >= REMD_CX_DISTANCE && op <= REMD_CX_DIHEDRAL) { cx_st(S, sp++, lane, cst_particles_op(op, arg, seed, X, lane, Lx, Ly, Lz)); break; }
            const cx x = cx_ld(S, sp - 1, lane);
            double v = 0.0, k = 0.0;
            switch (op) {
            case REMD_CX_NEG:  v = -x.v; k = -1.0; break;
            case REMD_CX_POWI: {
                const int m = arg < 0 ? -arg : arg;
                const double pm1 = m > 0 ? cst_ipow(x.v, m - 1) : 0.0, pm = m > 0 ? pm1 * x.v : 1.0;
                if (arg >= 0) { v = pm; k = (double)m * pm1; }
                else { v = 1.0 / pm; k = -(double)m * v / x.v; }
            } break;
            case REMD_CX_SQRT: v = sqrt(x.v); k = v > 0.0 ? 0.5 / v : 0.0; break;
            case REMD_CX_EXP:  v = exp(x.v); k = v; break;
            case REMD_CX_LOG:  v = log(x.v); k = 1.0 / x.v; break;
            case REMD_CX_SIN:  v = sin(x.v); k = cos(x.v); break;
            case REMD_CX_COS:  v = cos(x.v); k = -sin(x.v); break;
            case REMD_CX_TAN:  v = tan(x.v); k = 1.0 + v * v; break;
            case REMD_CX_ASIN: v = asin(x.v); k = 1.0 / sqrt(1.0 - x.v * x.v); break;
            case REMD_CX_ACOS: v = acos(x.v); k = -1.0 / sqrt(1.0 - x.v * x.v); break;
            case REMD_CX_ATAN: v = atan(x.v); k = 1.0 / (1.0 + x.v * x.v); break;
            case REMD_CX_SINH: v = sinh(x.v); k = cosh(x.v); break;
            case REMD_CX_COSH: v = cosh(x.v); k = sinh(x.v); break;
            case REMD_CX_TANH: v = tanh(x.v); k = 1.0 - v * v; break;
            case REMD_CX_ERF:  v = erf(x.v); k = 1.1283791670955126 * exp(-x.v * x.v); break;
            case REMD_CX_ERFC: v = erfc(x.v); k = -1.1283791670955126 * exp(-x.v * x.v); break;
            case REMD_CX_ABS:  v = fabs(x.v); k = x.v < 0.0 ? -1.0 : 1.0; break;
            case REMD_CX_STEP: v = x.v >= 0.0 ? 1.0 : 0.0; break;
            case REMD_CX_DELTA: v = x.v == 0.0 ? 1.0 : 0.0; break;
            case REMD_CX_FLOOR: v = floor(x.v); break;
            case REMD_CX_CEIL: v = ceil(x.v); break;
            case REMD_CX_TABLE1D: cst_table1d(consts + f.const0 + arg, x.v, v, k); break;
            case REMD_CX_LOOKUP1D: v = cst_lookup1d(consts + f.const0 + arg, x.v); break;
            default: break;
            }
            cx_st(S, sp - 1, lane, cx_chain(v, k, x));
        } break;
        }
    }
    return cx_ld(S, 0, lane);
}

__device__ __forceinline__ double cst_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace

// custom_compound.hip: the launches of the compound-bond forces' wavefronts (the part CST_COMPOUND), on the stream and between the
// launches of remd_custom_forces / remd_custom_ukl
void remd_custom_compound_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st);
void remd_custom_compound_ukl(remd_ctx* h, cst_tables& t);
// (the *_dpar launches: D[r][d][w] of the declared energy parameter derivatives -> d_dD, on the main stream; states: D[r][l][d][w]
// under every state's globals -> d_dDK)
void remd_custom_compound_dpar(remd_ctx* h, cst_tables& t, bool states);
// custom_centroid.hip: the same for the centroid forces' wavefronts (the part CST_CENTROID): centroids, bonds, spread
void remd_custom_centroid_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st);
void remd_custom_centroid_ukl(remd_ctx* h, cst_tables& t);
void remd_custom_centroid_dpar(remd_ctx* h, cst_tables& t, bool states);
// custom_cv.hip: the same for the collective-variable forces' wavefronts (the part CST_CV): superposition, expression, spread
void remd_custom_cv_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st);
void remd_custom_cv_ukl(remd_ctx* h, cst_tables& t);
size_t remd_custom_cv_w();             // doubles per (replica, variable) of cst_tables::d_W; the RMSD is the first
// cmap.hip: the force launch of the CMAP forces' wavefronts (the part CST_CMAP); they have no globals, so no u_kl launch
void remd_cmap_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st);
// custom_nonbonded.hip: the same for the nonbonded forces' tiles (the part CST_NONBONDED), and the long-range
// correction's share of the energies (behind custom_reduce_kernel) and of the u_kl rows (behind custom_ukl_reduce_kernel)
void remd_custom_nonbonded_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st);
void remd_custom_nonbonded_lrc(remd_ctx* h, cst_tables& t, int ep_slot, hipStream_t st);
void remd_custom_nonbonded_ukl(remd_ctx* h, cst_tables& t);
void remd_custom_nonbonded_lrc_ukl(remd_ctx* h, cst_tables& t, double* d_rows);
// custom_hbond.hip: the same for the donor-acceptor forces' tiles (the part CST_HBOND)
void remd_custom_hbond_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st);
void remd_custom_hbond_ukl(remd_ctx* h, cst_tables& t);
void remd_custom_hbond_dpar(remd_ctx* h, cst_tables& t, bool states);
// custom_manyparticle.hip: the same for the many-particle forces' central particles (the part CST_MANYPARTICLE, the last one): the
// neighbour rows, then the sets
void remd_custom_manyparticle_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st);
void remd_custom_manyparticle_ukl(remd_ctx* h, cst_tables& t);
void remd_custom_manyparticle_dpar(remd_ctx* h, cst_tables& t, bool states);
// custom_gb.hip: the same for the Generalized-Born forces (the part CST_GB, the last one): five launches per force.  They carry no
// globals, so they have no u_kl launch
void remd_custom_gb_forces(remd_ctx* h, cst_tables& t, bool with_energy, hipStream_t st);
