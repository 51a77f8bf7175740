// Listed terms (harmonic bonds, angles, periodic torsions, non-zero 1-4 exceptions, Ewald exclusion correction), one term per thread.
// Force-only evaluations: listed_forces_body, shared by forces.hip (listed_forces_kernel), resident.hip and pme.hip (round 4: in the
// mode in which the direct-space stream is the critical one the terms ride as extra workgroups of the spreading launch on the mesh
// stream -- one dependent 13 us launch less).  Evaluations with energies: bond_kernel, angle_kernel, exception_kernel and
// ewald_exclusion_kernel of forces.hip call the same <class>_term and sum the energy themselves.  Functional forms: OpenMM HarmonicBondForce / HarmonicAngleForce / PeriodicTorsionForce /
// NonbondedForce exceptions as the reference's test systems build them (testsystems.py:3504-3517); f64 restatement:
// oracle/forcefield.py.
#pragma once
#include "remd_internal.h"

__device__ __forceinline__ void add_force(long long* __restrict__ F, int Npad, int i, float fx, float fy, float fz)
{
    unsigned long long* U = reinterpret_cast<unsigned long long*>(F);
    atomicAdd(&U[i],            remd_f2fix(fx));
    atomicAdd(&U[Npad + i],     remd_f2fix(fy));
    atomicAdd(&U[2 * Npad + i], remd_f2fix(fz));
}


__device__ __forceinline__ float3 ld3(const float4* P, int i) { const float4 p = P[i]; return make_float3(p.x, p.y, p.z); }
__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 scl3(float3 a, float s) { return make_float3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float3 add3(float3 a, float3 b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ float dotf(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float3 crs3(float3 a, float3 b) {
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}



// Lennard-Jones part of an exception between an alchemical and a non-alchemical atom: the factory moves it to a
// lambda_sterics-controlled CustomBondForce with the soft-core expression of the pair interactions, no cutoff, no switch
// (alchemy.py:1836-1851, 1985-1998, expression :1374-1380 with softcore_c = 6).  lam_a = lambda^a, sc = alpha (1 - lambda)^b.
// Returns (U, dU/dr).
__device__ __forceinline__ float2 softcore_exception(float lam_a, float sc, float sig, float eps, float r2, float inv_r)
{
    const float is2 = 1.f / (sig * sig);
    const float t = r2 * r2 * r2 * is2 * is2 * is2;
    const float x = 1.f / (sc + t);
    const float e4 = 4.f * eps * lam_a;
    return make_float2(e4 * x * (x - 1.f), e4 * (2.f * x - 1.f) * (-x * x * 6.f * t * inv_r));
}


// ---- the terms, one statement per class.  <class>_term is the arithmetic: it takes the term's atom indices and parameters as values,
// leaves the forces on every atom of the term in `o` (slot order = the order of its atom indices) and returns what a caller needs to
// form the energy in its own precision (forces.hip: f64 sums).  listed_<class> reads the values of
// term t from listed_tables.  Every caller adds exactly the same fixed-point forces; one that does not use the forces, or the
// returned value, leaves that part to dead-code elimination.
// (named members, no arrays: a slot picked at run time from an array would put the array into scratch memory)
struct listed_out { int a0, a1, a2, a3; float f0x, f0y, f0z, f1x, f1y, f1z, f2x, f2y, f2z, f3x, f3y, f3z; };
#define LISTED_SET(o, k, X, Y, Z) do { (o).f##k##x = (X); (o).f##k##y = (Y); (o).f##k##z = (Z); } while (0)
// the forces of a term's first n atoms into the fixed-point accumulator of one replica
__device__ __forceinline__ void listed_add(long long* __restrict__ F, int Npad, const listed_out& o, int n)
{
    add_force(F, Npad, o.a0, o.f0x, o.f0y, o.f0z);
    add_force(F, Npad, o.a1, o.f1x, o.f1y, o.f1z);
    if (n > 2) add_force(F, Npad, o.a2, o.f2x, o.f2y, o.f2z);
    if (n > 3) add_force(F, Npad, o.a3, o.f3x, o.f3y, o.f3z);
}
// an angle's forces, ends first, for the caller that has always added them so (angle_kernel of forces.hip).  The
// integer sums do not care, the compiler does: it pairs the products behind the atomics into packed multiplies and FMAs in the order
// it meets them, and another order contracts other products -- other last bits of that caller's forces.
__device__ __forceinline__ void listed_add_angle(long long* __restrict__ F, int Npad, const listed_out& o)
{
    add_force(F, Npad, o.a0, o.f0x, o.f0y, o.f0z);
    add_force(F, Npad, o.a2, o.f2x, o.f2y, o.f2z);
    add_force(F, Npad, o.a1, o.f1x, o.f1y, o.f1z);
}

// harmonic bond 0.5 k (len - r0)^2; returns len - r0
__device__ __forceinline__ float bond_term(int i, int j, float r0, float k, const float4* __restrict__ P, listed_out& o)
{
    const float3 d = sub3(ld3(P, j), ld3(P, i));
    const float len = sqrtf(dotf(d, d));
    const float dl = len - r0;
    const float fs = k * dl / len;                   // F_i = +fs * d, F_j = -fs * d
    o.a0 = i; o.a1 = j;
    LISTED_SET(o, 0, fs * d.x, fs * d.y, fs * d.z);
    LISTED_SET(o, 1, -fs * d.x, -fs * d.y, -fs * d.z);
    return dl;
}
// harmonic angle 0.5 k (theta - th0)^2 at b; returns theta - th0
__device__ __forceinline__ float angle_term(int a, int b, int c, float th0, float k, const float4* __restrict__ P, listed_out& o)
{
    const float3 v0 = sub3(ld3(P, a), ld3(P, b)), v1 = sub3(ld3(P, c), ld3(P, b));      // b -> a, b -> c
    const float3 cp = crs3(v0, v1);
    const float rp = fmaxf(sqrtf(dotf(cp, cp)), 1e-6f);
    const float r20 = dotf(v0, v0), r21 = dotf(v1, v1);
    const float cosine = fminf(fmaxf(dotf(v0, v1) * rsqrtf(r20 * r21), -1.f), 1.f);
    const float dth = acosf(cosine) - th0;
    const float dEdth = k * dth;
    // dtheta/dx_a = (v0 x cp) / (|v0|^2 |cp|),  dtheta/dx_c = (cp x v1) / (|v1|^2 |cp|)
    const float3 fa = scl3(crs3(v0, cp), -dEdth / (r20 * rp));
    const float3 fc = scl3(crs3(cp, v1), -dEdth / (r21 * rp));
    o.a0 = a; o.a1 = b; o.a2 = c;
    LISTED_SET(o, 0, fa.x, fa.y, fa.z); LISTED_SET(o, 2, fc.x, fc.y, fc.z);
    LISTED_SET(o, 1, -(fa.x + fc.x), -(fa.y + fc.y), -(fa.z + fc.z));
    return dth;
}
// periodic torsion k (1 + cos(per phi - phase)); returns per phi - phase
__device__ __forceinline__ float torsion_term(int a1, int a2, int a3, int a4, float per, float phase, float k, const float4* __restrict__ P,
                                              listed_out& o)
{
    const float3 p1 = ld3(P, a1), p2 = ld3(P, a2), p3 = ld3(P, a3), p4 = ld3(P, a4);
    const float3 b1 = sub3(p2, p1), b2 = sub3(p3, p2), b3 = sub3(p4, p3);
    const float3 m = crs3(b1, b2), nn = crs3(b2, b3);
    const float m2 = fmaxf(dotf(m, m), 1e-12f), n2 = fmaxf(dotf(nn, nn), 1e-12f);
    const float lb2 = sqrtf(dotf(b2, b2));
    // IUPAC dihedral: phi = atan2(|b2| b1.(b2 x b3), (b1 x b2).(b2 x b3))
    const float phi = atan2f(lb2 * dotf(b1, nn), dotf(m, nn));
    const float arg = per * phi - phase;
    const float dEdphi = -k * per * sinf(arg);
    // gradient of phi (Blondel & Karplus 1996)
    const float3 g1 = scl3(m, -lb2 / m2);
    const float3 g4 = scl3(nn, lb2 / n2);
    const float s12 = dotf(b1, b2) / (lb2 * lb2), s32 = dotf(b3, b2) / (lb2 * lb2);
    const float3 g2 = add3(scl3(g1, -(1.f + s12)), scl3(g4, s32));     // = -g1 - s12 g1 + s32 g4
    const float3 g3 = add3(scl3(g4, -(1.f + s32)), scl3(g1, s12));
    o.a0 = a1; o.a1 = a2; o.a2 = a3; o.a3 = a4;
    LISTED_SET(o, 0, -dEdphi * g1.x, -dEdphi * g1.y, -dEdphi * g1.z);
    LISTED_SET(o, 1, -dEdphi * g2.x, -dEdphi * g2.y, -dEdphi * g2.z);
    LISTED_SET(o, 2, -dEdphi * g3.x, -dEdphi * g3.y, -dEdphi * g3.z);
    LISTED_SET(o, 3, -dEdphi * g4.x, -dEdphi * g4.y, -dEdphi * g4.z);
    return arg;
}
// 1-4 style exception with non-zero parameters: plain Coulomb + LJ, no cutoff, no switch; returns U.  L: the box edges (L.x <= 0: no
// box).  lam: the replica's row of rep_lam (NULL: no alchemy), alch: the pair's alchemical atoms -- > 0 scales the charge product
// (alchemy.py:1964-1966 exception offset), 1 with eps != 0 takes the soft-core.
__device__ __forceinline__ float exception_term(int i, int j, float qq, float sig, float eps, int alch, const float* __restrict__ lam, float3 L,
                                                const float4* __restrict__ P, listed_out& o)
{
    if (lam && alch > 0) qq *= lam[2];
    float3 d = sub3(ld3(P, j), ld3(P, i));
    if (L.x > 0.f) { d.x -= L.x * rintf(d.x / L.x); d.y -= L.y * rintf(d.y / L.y); d.z -= L.z * rintf(d.z / L.z); }
    const float r2 = dotf(d, d);
    const float inv_r = rsqrtf(r2);
    float Ulj, dUlj;
    if (lam && alch == 1 && eps != 0.f) {
        const float2 sc = softcore_exception(lam[0], lam[1], sig, eps, r2, inv_r);
        Ulj = sc.x; dUlj = sc.y;
    } else {
        const float s2 = sig * sig * inv_r * inv_r, s6 = s2 * s2 * s2;
        Ulj = 4.f * eps * s6 * (s6 - 1.f); dUlj = 4.f * eps * s6 * (6.f - 12.f * s6) * inv_r;
    }
    const float U = Ulj + qq * inv_r;
    const float dUdr = dUlj - qq * inv_r * inv_r;
    const float fr = dUdr * inv_r;
    o.a0 = i; o.a1 = j;
    LISTED_SET(o, 0, fr * d.x, fr * d.y, fr * d.z);
    LISTED_SET(o, 1, -fr * d.x, -fr * d.y, -fr * d.z);
    return U;
}
// Ewald correction for an excluded pair: the reciprocal sum contains it, so subtract qq erf(alpha r)/r; returns U.  alch alchemical
// atoms scale the charge product by lambda_electrostatics^alch.
// R_FIRST: alpha r is formed as alpha (r2 / r) instead of (alpha r2) / r.  The evaluations with energies have always rounded it the
// first way and the force-only ones the second; the two differ in the last bit, and each caller keeps its own.
template <bool R_FIRST>
__device__ __forceinline__ float exclusion_term(int i, int j, float qq, int alch, const float* __restrict__ lam, float3 L, float alpha,
                                                float two_alpha_sqrtpi, const float4* __restrict__ P, listed_out& o)
{
    if (lam) { const float le = lam[2]; qq *= (alch == 2) ? le * le : (alch == 1) ? le : 1.f; }
    float3 d = sub3(ld3(P, j), ld3(P, i));
    d.x -= L.x * rintf(d.x / L.x); d.y -= L.y * rintf(d.y / L.y); d.z -= L.z * rintf(d.z / L.z);
    const float r2 = dotf(d, d);
    const float inv_r = rsqrtf(r2);
    const float ar = R_FIRST ? alpha * (r2 * inv_r) : alpha * r2 * inv_r;
    const float erf_ar = erff(ar);
    const float U = -qq * erf_ar * inv_r;
    const float dUdr = -qq * (two_alpha_sqrtpi * __expf(-ar * ar) * inv_r - erf_ar * inv_r * inv_r);
    const float fr = dUdr * inv_r;
    o.a0 = i; o.a1 = j;
    LISTED_SET(o, 0, fr * d.x, fr * d.y, fr * d.z);
    LISTED_SET(o, 1, -fr * d.x, -fr * d.y, -fr * d.z);
    return U;
}

// the loaders: term t of listed_tables, replica r
__device__ __forceinline__ void listed_bond(const listed_tables& T, int t, const float4* __restrict__ P, listed_out& o)
{
    bond_term(T.bond_atoms[2 * t], T.bond_atoms[2 * t + 1], T.bond_params[2 * t], T.bond_params[2 * t + 1], P, o);
}
__device__ __forceinline__ void listed_angle(const listed_tables& T, int t, const float4* __restrict__ P, listed_out& o)
{
    angle_term(T.angle_atoms[3 * t], T.angle_atoms[3 * t + 1], T.angle_atoms[3 * t + 2], T.angle_params[2 * t], T.angle_params[2 * t + 1], P, o);
}
__device__ __forceinline__ void listed_torsion(const listed_tables& T, int t, const float4* __restrict__ P, listed_out& o)
{
    torsion_term(T.torsion_atoms[4 * t], T.torsion_atoms[4 * t + 1], T.torsion_atoms[4 * t + 2], T.torsion_atoms[4 * t + 3],
                 T.torsion_params[3 * t], T.torsion_params[3 * t + 1], T.torsion_params[3 * t + 2], P, o);
}
__device__ __forceinline__ float3 box_edges(const float* __restrict__ box, int r) { return make_float3(box[4 * r], box[4 * r + 1], box[4 * r + 2]); }
__device__ __forceinline__ void listed_exception(const listed_tables& T, int t, const float4* __restrict__ P, const float* __restrict__ box, int r,
                                                 listed_out& o)
{
    const float* lam = T.rep_lam ? T.rep_lam + 4 * r : nullptr;
    exception_term(T.exc_atoms[2 * t], T.exc_atoms[2 * t + 1], T.exc_params[3 * t], T.exc_params[3 * t + 1], T.exc_params[3 * t + 2],
                   lam ? T.exc_alch[t] : 0, lam, box_edges(box, r), P, o);
}
__device__ __forceinline__ void listed_exclusion(const listed_tables& T, int t, const float4* __restrict__ P, const float* __restrict__ box, int r,
                                                 listed_out& o)
{
    const float* lam = T.rep_lam ? T.rep_lam + 4 * r : nullptr;
    exclusion_term<false>(T.excl_atoms[2 * t], T.excl_atoms[2 * t + 1], T.excl_qq[t], lam ? T.excl_alch[t] : 0, lam, box_edges(box, r),
                          T.alpha, T.two_alpha_sqrtpi, P, o);
}

// All short "listed" terms of one force evaluation in a single launch (force-only path): harmonic bonds, angles,
// periodic torsions, non-zero exceptions and the Ewald exclusion correction.
//
// Two organisations of the same arithmetic.  One TERM per thread (T.aterm NULL): every atom of the term gets its three integer
// atomics -- 6 to 12 scattered 64-bit atomics per term, and scattered atomics are what that launch spends its time on (MI355X:
// ~45 G per second chip-wide, ONE PER 64-BYTE LINE an instruction touches; DHFR x 16: 180 us with them, 6 without,
// profiles/r06_23_atomics_knock_out.txt).  Round 6, the default: one (term, atom of the term) ENTRY per thread, the entries in the
// order of the atoms they act on (remd_ctx::d_aterm: class << 29 | slot << 27 | term, forces.hip: build_atom_terms): every thread
// evaluates the whole term and adds only its slot's force, so the 64 lanes of an atomic instruction fall on a handful of
// neighbouring atoms -- a few lines instead of 64 -- at the price of evaluating a torsion four times.  Integer sums do not
// depend on the order: the totals are the same fixed-point numbers.
__device__ __forceinline__
void listed_forces_body(const listed_tables& T, int Npad, const float4* __restrict__ pos, const float* __restrict__ box,
                        long long* __restrict__ force, int t, int r)
{
    const float4* P = pos + (size_t)r * Npad;
    long long* F = force + (size_t)r * 3 * Npad;
    int cls = -1, slot = -1;                              // slot -1: this thread adds every slot of the term
    if (T.aterm) {
        // (no early return on this path: every lane takes part in the reduction over the lanes of one atom below)
        if (t < T.n_aterm) {
            const unsigned int ent = T.aterm[t];
            cls = (int)(ent >> 29); slot = (int)((ent >> 27) & 3u); t = (int)(ent & 0x7ffffffu);
            const int n_cls = cls == 0 ? T.n_bonds : cls == 1 ? T.n_angles : cls == 2 ? T.n_torsions : cls == 3 ? T.n_exc : T.n_excl;
            if (n_cls == 0) cls = -1;                     // the class is not part of this evaluation (force groups)
        }
    } else {
        if (t < T.n_bonds) cls = 0;
        else if ((t -= T.n_bonds) < T.n_angles) cls = 1;
        else if ((t -= T.n_angles) < T.n_torsions) cls = 2;
        else if ((t -= T.n_torsions) < T.n_exc) cls = 3;
        else if ((t -= T.n_exc) < T.n_excl) cls = 4;
        else return;
    }
    listed_out o;
    o.a0 = o.a1 = o.a2 = o.a3 = 0;
    LISTED_SET(o, 0, 0.f, 0.f, 0.f); LISTED_SET(o, 1, 0.f, 0.f, 0.f); LISTED_SET(o, 2, 0.f, 0.f, 0.f); LISTED_SET(o, 3, 0.f, 0.f, 0.f);
    int n = 0;
    if (cls == 0) { listed_bond(T, t, P, o); n = 2; }
    else if (cls == 1) { listed_angle(T, t, P, o); n = 3; }
    else if (cls == 2) { listed_torsion(T, t, P, o); n = 4; }
    else if (cls == 3) { listed_exception(T, t, P, box, r, o); n = 2; }
    else if (cls == 4) { listed_exclusion(T, t, P, box, r, o); n = 2; }
    if (T.aterm) {
        // (the members are pinned to registers first: left alone the compiler turns the selects below into selects of the members'
        //  ADDRESSES and keeps the struct in scratch memory)
        int a0 = o.a0, a1 = o.a1, a2 = o.a2, a3 = o.a3;
        float f0x = o.f0x, f0y = o.f0y, f0z = o.f0z, f1x = o.f1x, f1y = o.f1y, f1z = o.f1z;
        float f2x = o.f2x, f2y = o.f2y, f2z = o.f2z, f3x = o.f3x, f3y = o.f3y, f3z = o.f3z;
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
        asm volatile("" : "+v"(f0x), "+v"(f0y), "+v"(f0z), "+v"(f1x), "+v"(f1y), "+v"(f1z));
        asm volatile("" : "+v"(f2x), "+v"(f2y), "+v"(f2z), "+v"(f3x), "+v"(f3y), "+v"(f3z));
        const int lane = (int)(threadIdx.x & 63u);
        int a = slot == 0 ? a0 : slot == 1 ? a1 : slot == 2 ? a2 : a3;
        const float fx = slot == 0 ? f0x : slot == 1 ? f1x : slot == 2 ? f2x : f3x;
        const float fy = slot == 0 ? f0y : slot == 1 ? f1y : slot == 2 ? f2y : f3y;
        const float fz = slot == 0 ? f0z : slot == 1 ? f1z : slot == 2 ? f2z : f3z;
        if (cls < 0) a = -1 - lane;                       // idle lane: a segment of its own, nothing to add
        // The entries are in atom order, so the lanes of one atom are neighbours: their fixed-point forces are summed along the
        // run (a segmented scan over the wavefront) and the run's last lane issues the atom's one atomic triple.  Atomics of
        // several lanes on ONE address are serialised at the L2 (measured: the entries with an atomic each are slower than the
        // term-per-thread launch), while the runs' last lanes hit distinct, neighbouring atoms.
        // A segment is a run of NEIGHBOURING lanes with one atom, bounded by head flags -- not "the lane d back has my atom".
        // Idle lanes sit inside an atom's run wherever a force-group evaluation switches a class off (an atom's entries are
        // bond, angle, torsion, exception, exclusion: bonds + torsions leave the angle lanes idle between them).  Such a lane
        // splits the run into two segments, each with its own atomic; a scan that compared atoms across the gap would add the
        // first segment's partial sum into the second as well, after the first had already sent it: that atom's force twice.
        const int ap = __shfl_up(a, 1);
        const unsigned long long heads = __ballot(lane == 0 || ap != a);
        const int s0 = 63 - __clzll(heads & (~0ull >> (63 - lane)));      // first lane of this lane's segment
        unsigned long long vx = cls < 0 ? 0ull : remd_f2fix(fx), vy = cls < 0 ? 0ull : remd_f2fix(fy), vz = cls < 0 ? 0ull : remd_f2fix(fz);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long ux = __shfl_up(vx, d), uy = __shfl_up(vy, d), uz = __shfl_up(vz, d);
            if (lane - d >= s0) { vx += ux; vy += uy; vz += uz; }
        }
        if (cls >= 0 && (lane == 63 || ((heads >> (lane + 1)) & 1ull))) {
            unsigned long long* U = reinterpret_cast<unsigned long long*>(F);
            atomicAdd(&U[a], vx); atomicAdd(&U[Npad + a], vy); atomicAdd(&U[2 * Npad + a], vz);
        }
        return;
    }
    listed_add(F, Npad, o, n);
}
