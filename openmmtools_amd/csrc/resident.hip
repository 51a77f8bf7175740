// Resident kernels (gfx950): small systems whose whole propagation -- every MD step of a move -- runs inside ONE launch, a workgroup
// per replica: resident_md_kernel (Lennard-Jones fluids, an atom per thread) and resident_mol_kernel (small molecules in vacuum, a
// constraint unit per thread with the unit arithmetic of constraint_units.h).  step_runner::begin (integrate.hip) offers every
// request to the two launchers at the end of this file first.
#include "constraint_units.h"
#include "pair_math.h"
#include "listed_terms.h"
#include "nocutoff_pair.h"

// ---------------------------------------------------------------------------------------------------------------------
// Resident small-system path (round 3).  For systems of up to 1024 atoms without constraints, mesh or listed terms (the
// reference's HarmonicOscillator and LennardJonesFluid test systems: BASELINE configs 1 and 2) an MD step of the regular path
// is a chain of ~8 dependent launches of a few microseconds each and the GPU idles in between (LJ fluid, 16 replicas: 30 us
// per step for 8 k atoms).  mcmc.py:700-719 is ONE integrator.step(n_steps) per move, so the MI355X-first shape of that is
// ONE launch per propagation: a workgroup owns a replica, a thread owns an atom (x, v, f, 1/m and the pair parameters stay in
// registers for all n_steps), positions and a Verlet list live in LDS:
//   * neighbour list: all pairs inside r_c + skin, FULL list (every pair from both sides: no atomics, every atom sums its
//     forces in list order -- deterministic), rebuilt by an all-pairs pass over the LDS positions whenever any atom has moved
//     more than skin / 2 since the last build (a workgroup vote at every evaluation): the list is a superset of the pairs
//     inside r_c at all times, the cutoff test in the force loop is exact;
//   * force evaluation where the splitting string needs one (a V after an R), with the pair arithmetic of the regular
//     kernels (pair_math.h: LJ + switch, soft-core for alchemical / non-alchemical pairs at the replica's lambda);
//   * V / R / O / centre-of-mass removal as in the chain kernel, same Philox streams (atom, global replica, global O-substep
//     counter): the trajectories follow the regular path to fp32 summation order.
// Two workgroup barriers per force evaluation, nothing else between steps.
struct resident_prog : step_prog {
    int n_steps, cmm_frequency; long long gstep0, first_step;
};
struct resident_sys {
    int N, Npad, method, alch, n_ext, list_cap;
    nb_params p;
    float skin, ext_K, ext_x0, inv_total_mass;
    const float4* param; const float* rep_lam; const int* ext_atoms; const float* invmass; const float* box;
    const int64_t* labels; const double* beta; int r_begin; uint64_t seed; const unsigned int* noise_id;
    unsigned int* err;
};

#ifndef RES_UNROLL
#define RES_UNROLL 2
#endif
#define RES_FSCALE 8192.f       // LDS force accumulators: 32-bit fixed point, 2^-13 kJ/mol/nm (|F| < 2.6e5 kJ/mol/nm: r > 0.19 nm for argon)

// LJ + switch of one pair without branches: the soft-core form  x = 1 / (sc + (r / sigma)^6),  U = lam eps4 x (x - 1)  IS
// Lennard-Jones for sc = 0, lam = 1 (alchemy.py:1383-1388 with softcore_c = 6), so alchemical / non-alchemical pairs differ from
// the rest only in two selected constants; the switching polynomial is evaluated at x clamped to [0, 1].  Hardware reciprocals
// (1 ulp).  Returns dU/dr / r, so that F_i = fr * (x_j - x_i).
template <bool ALCH>
__device__ __forceinline__ float resident_pair(const nb_params& p, float r2, float4 pi, float4 pj, float lam_a, float sc)
{
    const float inv_r = __builtin_amdgcn_rsqf(r2), r = r2 * inv_r;
    const float sig = pi.y + pj.y, eps4 = pi.z * pj.z;
    const bool soft = ALCH && ((pi.w != pj.w) || pi.w > 1.5f);      // (w = 2: annihilate_sterics, pair_math.h)
    const float lam = soft ? lam_a : 1.f, s0 = soft ? sc : 0.f;
    const float is2 = __builtin_amdgcn_rcpf(sig * sig);
    const float q2 = r2 * is2, t = q2 * q2 * q2;
    const float x = __builtin_amdgcn_rcpf(s0 + t);
    float U = lam * eps4 * x * (x - 1.f);
    float dUdr = lam * eps4 * (2.f * x - 1.f) * (-x * x * 6.f * t * inv_r);
    const float xs = fminf(fmaxf((r - p.rs) * p.inv_sw, 0.f), 1.f);          // no switch: inv_sw = 0
    const float Sw = 1.f + xs * xs * xs * (-10.f + xs * (15.f - 6.f * xs));
    const float dS = xs * xs * (-30.f + xs * (60.f - 30.f * xs)) * p.inv_sw;
    dUdr = Sw * dUdr + U * dS;
    return dUdr * inv_r;
}

template <bool ALCH>
__global__ __launch_bounds__(1024)
void resident_md_kernel(resident_prog prog, resident_sys S, float4* __restrict__ pos, float4* __restrict__ vel)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int N = S.N, T = blockDim.x, tid = threadIdx.x, r = blockIdx.x, nw = T >> 6;
    float4* s_pos = reinterpret_cast<float4*>(smem);                      // [T] positions (w: unused)
    float4* s_par = s_pos + T;                                            // [T] pair parameters of every atom
    float* s_red = reinterpret_cast<float*>(s_par + T);                   // [16][4] wavefront partial sums; the last words:
    int* s_vote = reinterpret_cast<int*>(s_red + 60);                     // [2] "somebody left its skin / 2 sphere", by evaluation parity
    int* s_np = reinterpret_cast<int*>(s_red + 62);                       // pairs in the list
    int* s_f = reinterpret_cast<int*>(s_red + 64);                        // [3][T] fixed-point force accumulators
    unsigned long long* s_fl = reinterpret_cast<unsigned long long*>(s_f + 3 * T + (T & 1));   // [3][T] the same in 64 bits: contributions too large for the fast path
    unsigned int* s_pairs = reinterpret_cast<unsigned int*>(s_fl + 3 * T); // [cap] i | j << 16, i < j
    const bool active = tid < N;
    float4* P = pos + (size_t)r * S.Npad;
    float4* V = vel + (size_t)r * S.Npad;
    float3 x = f3(0, 0, 0), v = f3(0, 0, 0), f = f3(0, 0, 0), xref = f3(0, 0, 0);
    float im = 0.f;
    float4 par = make_float4(0, 0, 0, 0);
    if (active) {
        const float4 p4 = P[tid], v4 = V[tid];
        x = f3(p4.x, p4.y, p4.z); v = f3(v4.x, v4.y, v4.z);
        im = S.invmass[tid];
        if (S.method >= 0) par = S.param[tid];
    }
    s_par[tid] = par;
    s_f[tid] = 0; s_f[T + tid] = 0; s_f[2 * T + tid] = 0;
    s_fl[tid] = 0ull; s_fl[T + tid] = 0ull; s_fl[2 * T + tid] = 0ull;
    bool ext = false;
    for (int k = 0; k < S.n_ext; ++k) ext |= (S.ext_atoms[k] == tid);
    const float Lx = S.box[4 * r], Ly = S.box[4 * r + 1], Lz = S.box[4 * r + 2];
    const float iLx = Lx > 0.f ? 1.f / Lx : 0.f, iLy = Ly > 0.f ? 1.f / Ly : 0.f, iLz = Lz > 0.f ? 1.f / Lz : 0.f;
    float lam_a = 1.f, sc = 0.f;
    if (ALCH) { lam_a = S.rep_lam[4 * r]; sc = S.rep_lam[4 * r + 1]; }
    const float kT = frcp((float)S.beta[S.labels[S.r_begin + r]]);
    const uint32_t rg = S.noise_id ? S.noise_id[r] : (uint32_t)(S.r_begin + r);
    const float rl = S.p.rc + S.skin, rl2 = rl * rl, half_skin2 = 0.25f * S.skin * S.skin;
    bool have_list = false, forces_valid = false;
    int n_eval = 0;
    if (tid == 0) { s_vote[0] = 0; s_vote[1] = 0; *s_np = 0; }
    __syncthreads();

    auto evaluate = [&]() {
        // publish the positions; rebuild the list if any atom has left its skin / 2 sphere.  The vote rides on the barrier that
        // publishes the positions (two words used in turn: the one of the next evaluation is cleared behind this barrier)
        const float3 d = x - xref;
        const bool moved = !have_list || (active && dot3(d, d) > half_skin2);
        const int par_e = n_eval & 1;
        s_pos[tid] = make_float4(x.x, x.y, x.z, 0.f);
        if (moved) s_vote[par_e] = 1;
        __syncthreads();
        const int rebuild = s_vote[par_e];
        if (tid == 0) s_vote[par_e ^ 1] = 0;
        ++n_eval;
        f = f3(0, 0, 0);
        if (S.method >= 0) {
            if (rebuild) {
                if (tid == 0) *s_np = 0;
                __syncthreads();
                if (active) {
                    for (int j = 0; j < N; ++j) {                        // wave-uniform j: LDS broadcast reads
                        const float4 q = s_pos[j];
                        float dx = q.x - x.x, dy = q.y - x.y, dz = q.z - x.z;
                        dx -= Lx * rintf(dx * iLx); dy -= Ly * rintf(dy * iLy); dz -= Lz * rintf(dz * iLz);
                        const float r2 = dx * dx + dy * dy + dz * dz;
                        if (r2 < rl2 && j > tid) {                       // every pair once; the order of the list does not matter
                            const int slot = atomicAdd(s_np, 1);         // (forces are integer sums)
                            if (slot < S.list_cap) s_pairs[slot] = (unsigned int)tid | ((unsigned int)j << 16);
                        }
                    }
                    xref = x;
                }
                have_list = true;
                __syncthreads();
                if (tid == 0 && *s_np > S.list_cap) atomicCAS(S.err, 0u, 4u);
            }
            {
                // a thread takes pairs tid, tid + T, ...: the same number for every lane (an atom-per-lane loop runs as long as the
                // busiest atom of the wavefront: 16 slots for 10 neighbours on average), RES_UNROLL pairs per trip with all their
                // LDS reads in flight
                const int np = min(*s_np, S.list_cap);
                for (int k = tid; k < np; k += RES_UNROLL * T) {
                    unsigned int w[RES_UNROLL]; float4 qi[RES_UNROLL], qj[RES_UNROLL], pi[RES_UNROLL], pj[RES_UNROLL];
#pragma unroll
                    for (int u = 0; u < RES_UNROLL; ++u) w[u] = s_pairs[min(k + u * T, np - 1)];
#pragma unroll
                    for (int u = 0; u < RES_UNROLL; ++u) {
                        const int i = w[u] & 0xffffu, j = w[u] >> 16;
                        qi[u] = s_pos[i]; qj[u] = s_pos[j]; pi[u] = s_par[i]; pj[u] = s_par[j];
                    }
#pragma unroll
                    for (int u = 0; u < RES_UNROLL; ++u) {
                        const int i = w[u] & 0xffffu, j = w[u] >> 16;
                        float dx = qj[u].x - qi[u].x, dy = qj[u].y - qi[u].y, dz = qj[u].z - qi[u].z;
                        dx -= Lx * rintf(dx * iLx); dy -= Ly * rintf(dy * iLy); dz -= Lz * rintf(dz * iLz);
                        const float r2 = dx * dx + dy * dy + dz * dz;
                        if (r2 < S.p.rc2 && k + u * T < np) {
                            const float fr = resident_pair<ALCH>(S.p, r2, pi[u], pj[u], lam_a, sc) * RES_FSCALE;
                            const float ax = fr * dx, ay = fr * dy, az = fr * dz;                                    // F_i = fr (x_j - x_i)
                            if (fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fabsf(az)) < 134217728.f) {                       // 2^27: sixteen of them fit 32 bits
                                const int fx = __float2int_rn(ax), fy = __float2int_rn(ay), fz = __float2int_rn(az);
                                atomicAdd(&s_f[i], fx); atomicAdd(&s_f[T + i], fy); atomicAdd(&s_f[2 * T + i], fz);
                                atomicAdd(&s_f[j], -fx); atomicAdd(&s_f[T + j], -fy); atomicAdd(&s_f[2 * T + j], -fz);
                            } else {
                                // a pair deep inside the repulsive core (an unminimised start): 64-bit accumulators, rare and slow
                                const long long fx = (long long)ax, fy = (long long)ay, fz = (long long)az;
                                atomicAdd(&s_fl[i], (unsigned long long)fx); atomicAdd(&s_fl[T + i], (unsigned long long)fy); atomicAdd(&s_fl[2 * T + i], (unsigned long long)fz);
                                atomicAdd(&s_fl[j], (unsigned long long)(-fx)); atomicAdd(&s_fl[T + j], (unsigned long long)(-fy)); atomicAdd(&s_fl[2 * T + j], (unsigned long long)(-fz));
                            }
                        }
                    }
                }
            }
            __syncthreads();                                 // every pair is in; nobody reads s_pos any more
            {
                const long long lx = (long long)s_fl[tid], ly = (long long)s_fl[T + tid], lz = (long long)s_fl[2 * T + tid];
                f = f3((float)s_f[tid], (float)s_f[T + tid], (float)s_f[2 * T + tid]);
                if (lx | ly | lz) {
                    f = f + f3((float)lx, (float)ly, (float)lz);
                    s_fl[tid] = 0ull; s_fl[T + tid] = 0ull; s_fl[2 * T + tid] = 0ull;
                }
                f = f * (1.f / RES_FSCALE);
            }
            s_f[tid] = 0; s_f[T + tid] = 0; s_f[2 * T + tid] = 0;      // (the next accumulation starts behind the next publication barrier)
        } else {
            __syncthreads();
        }
        if (ext) { f.x -= S.ext_K * (x.x - S.ext_x0); f.y -= S.ext_K * x.y; f.z -= S.ext_K * x.z; }
        forces_valid = true;
    };

    for (int s = 0; s < prog.n_steps; ++s) {
        const long long gstep = prog.gstep0 + s;
        if (prog.cmm_frequency > 0 && ((prog.first_step + s) % prog.cmm_frequency) == 0) {
            // integrators.py:1313: CMMotionRemover at the top of a step: v -= sum(m v) / M; fixed-order sums (deterministic)
            float3 pm = active ? v * frcp(im) : f3(0, 0, 0);
            for (int off = 32; off > 0; off >>= 1) { pm.x += __shfl_xor(pm.x, off); pm.y += __shfl_xor(pm.y, off); pm.z += __shfl_xor(pm.z, off); }
            if ((tid & 63) == 0) { s_red[3 * (tid >> 6)] = pm.x; s_red[3 * (tid >> 6) + 1] = pm.y; s_red[3 * (tid >> 6) + 2] = pm.z; }
            __syncthreads();
            float3 tot = f3(0, 0, 0);
            for (int w = 0; w < nw; ++w) tot = tot + f3(s_red[3 * w], s_red[3 * w + 1], s_red[3 * w + 2]);
            __syncthreads();
            if (active) v = v - tot * S.inv_total_mass;
        }
        for (int t = 0; t < prog.n; ++t) {
            const char tok = prog.tok[t];
            if (tok == 'V') {
                if (!forces_valid) evaluate();
                v = v + f * (prog.hV * im);
            } else if (tok == 'R') {
                x = x + v * prog.hR;
                forces_valid = false;
            } else {
                const uint64_t cnt = (uint64_t)gstep * (uint64_t)prog.nO + (uint64_t)prog.o_index[t];
                const float3 xi = gaussian3(S.seed, REMD_STREAM_OU, (uint32_t)tid, rg, cnt);
                const float sig = prog.b * fsqrt(kT * im);
                v = f3(prog.a * v.x + sig * xi.x, prog.a * v.y + sig * xi.y, prog.a * v.z + sig * xi.z);
            }
        }
    }
    if (active) {
        P[tid] = make_float4(x.x, x.y, x.z, 0.f);
        V[tid] = make_float4(v.x, v.y, v.z, 0.f);
    }
}

// what both resident kernels ask of a request: the path switched on, no barostat, no per-launch profiling, a program of V / R / O
// tokens that fits the kernel argument, no heat / shadow work
static bool resident_takes_request(const remd_ctx* h, const std::vector<char>& tokens, int n_steps)
{
    if (!h->sw.resident || h->no_resident || h->n_vsites > 0) return false;      // (the resident kernels know nothing of virtual sites)
    if (h->baro_frequency > 0 || h->profiling == 2 || (int)tokens.size() > MAX_TOK || n_steps < 1) return false;
    if (h->measure_heat || h->measure_shadow) return false;
    for (char c : tokens) if (c != 'V' && c != 'R' && c != 'O') return false;
    return true;
}

// the program of a propagation: n_steps steps from step first_step of this iteration
static resident_prog resident_program(const remd_ctx* h, const std::vector<char>& tokens, int nV, int nR, int nO,
                                      int64_t iteration, int64_t first_step, int n_steps)
{
    resident_prog prog{};
    remd_step_prog_fill(prog, tokens, h->dt, h->gamma, nV, nR, nO);
    prog.n_steps = n_steps; prog.cmm_frequency = h->cmm_frequency;
    prog.gstep0 = (long long)iteration * (long long)h->n_steps + first_step; prog.first_step = first_step;
    return prog;
}

// the Lennard-Jones kernel
int remd_run_steps_resident(remd_ctx* h, const std::vector<char>& tokens, int nV, int nR, int nO,
                            int64_t iteration, int64_t first_step, int n_steps)
{
    if (!resident_takes_request(h, tokens, n_steps)) return 0;
    if (h->N > 1024 || h->n_settle > 0 || h->n_shake > 0 || h->n_bonds > 0 || h->n_angles > 0 || h->n_torsions > 0 || h->n_restraints > 0 || h->n_custom > 0 || h->gbsa) return 0;
    int ok = 0, method = -1, alch = 0; nb_params p{}; const float4* param = nullptr; const float* rep_lam = nullptr;
    int rc = remd_nb_resident_info(h, &ok, &method, &alch, &p, &param, &rep_lam);
    if (rc) return rc;
    if (!ok) return 0;
    resident_sys S{};
    S.N = h->N; S.Npad = h->Npad; S.method = method; S.alch = alch; S.n_ext = h->n_ext; S.p = p;
    // skin: a fifth of the cutoff, at most what keeps r_c + skin inside half the smallest box edge (minimum image)
    double lmin = 1e30;
    for (int r = 0; r < h->R; ++r) for (int k = 0; k < 3; ++k) lmin = std::min(lmin, h->box_host.size() >= (size_t)3 * (r + 1) ? h->box_host[3 * r + k] : 1e30);
    S.skin = method >= 0 ? (float)std::max(0.0, std::min(0.2 * p.rc, 0.5 * lmin - p.rc - 1e-3)) : 0.f;
    if (method >= 0 && !(0.5 * lmin > p.rc)) return 0;
    S.ext_K = (float)h->ext_K; S.ext_x0 = (float)h->ext_x0; S.inv_total_mass = (float)(h->total_mass > 0 ? 1.0 / h->total_mass : 0.0);
    S.param = param; S.rep_lam = rep_lam; S.ext_atoms = h->d_ext_atoms; S.invmass = h->d_invmass; S.box = h->d_box;
    S.labels = h->d_labels; S.beta = h->d_beta; S.r_begin = h->r_begin; S.seed = h->seed; S.err = h->d_sync + 2; S.noise_id = h->d_noise_id;
    const int T = std::max(64, (h->N + 63) / 64 * 64);
    // pair-list capacity from the LDS that is left: positions + parameters (32 B per thread), partial sums / flags, force accumulators
    const size_t fixed = (size_t)T * 32 + 64 * sizeof(float) + (size_t)T * 12 + 8 + (size_t)T * 24;
    const size_t lds_max = 144 * 1024;
    S.list_cap = method >= 0 ? (int)std::min<size_t>(32768, (lds_max - fixed) / 4) : 0;
    if (h->sw.resident_cap) S.list_cap = std::max(1, std::min(S.list_cap, h->sw.resident_cap));      // test hook: provoke the overflow path
    if (method >= 0 && S.list_cap < 4 * h->N && !h->sw.resident_cap) return 0;
    const size_t lds = fixed + (size_t)S.list_cap * 4;
    const resident_prog prog = resident_program(h, tokens, nV, nR, nO, iteration, first_step, n_steps);
    remd_launch_join_wait(h);
    remd_prof_scope ps(h, "resident_md");
    if (alch) {
        REMD_CHECK(h, hipFuncSetAttribute((const void*)resident_md_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        hipLaunchKernelGGL(resident_md_kernel<true>, dim3(h->R), dim3(T), lds, h->stream, prog, S, h->d_pos, h->d_vel);
    } else {
        REMD_CHECK(h, hipFuncSetAttribute((const void*)resident_md_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
        hipLaunchKernelGGL(resident_md_kernel<false>, dim3(h->R), dim3(T), lds, h->stream, prog, S, h->d_pos, h->d_vel);
    }
    REMD_CHECK(h, hipGetLastError());
    h->forces_valid = false; h->force_zeroed = false;
    remd_nb_invalidate_sort(h);            // the atoms moved n_steps without the regular path's evaluation counter seeing it
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Resident small-molecule MD (round 6): the reference's vacuum test systems (AlanineDipeptideVacuum 22 atoms, HostGuestVacuum 156,
// TolueneVacuum 15; testsystems.py:3352-3388) are three dependent launches per MD step on the regular path -- NoCutoff pair sum, listed
// terms, integrator chain -- of which the chain alone is 25 us of fixed latency for 22 atoms (rocprofv3, profiles/r06_43): 39 us per step
// whatever the size.  As for the Lennard-Jones fluids above, ONE launch per propagation: a workgroup owns a replica; a thread owns a
// constraint unit (x, v, 1/m of its <= 4 atoms in registers for all n_steps, the unit arithmetic of the chain kernel: X-H clusters,
// rigid waters, free atoms) AND, for the pair sum, an atom; positions, pair parameters and the fixed-point force accumulators live in LDS.
// A force evaluation is: units publish their positions and clear their atoms' accumulators | barrier | every atom sums its partners in
// ascending order (nocutoff_pair.h: the arithmetic and the order of nocutoff_kernel), exceptions, listed terms (listed_forces_body, the
// accumulators being an LDS address) | barrier.  Every contribution is converted to fixed point exactly as on the regular path and integer
// sums do not depend on their order; with the same Philox streams and the same centre-of-mass sum (per-wavefront fp32 partial sums in
// unit order, then integers) the trajectory follows the regular path to fp32 rounding (one step: velocities within 1 ulp, positions equal;
// the compiler contracts the long expressions of the two kernels differently; tools/experiments/resident_mol_diff.py), like the
// Lennard-Jones kernel above (tests/test_nocutoff.py::test_resident_small_molecule_kernel_follows_the_regular_launches).
// Measured (profiles/r06_43_small_molecule_systems.txt): 24 x AlanineDipeptideVacuum 39 -> 23 us per MD step; a step is then the latency
// of its seven tokens at one wavefront per SIMD (~1 us each, X-H Newton iterations) + one evaluation.  From ~100 atoms on one workgroup
// per replica loses against the regular launches, which spread the listed terms over the chip (CB7:B2 in vacuum, 156 atoms: 72 against
// 61 us per step) -- the kernel takes systems of up to RESIDENT_MOL_MAX_ATOMS atoms.
struct resident_mol_sys {
    int N, Npad, n_units, words, n_exc;
    const float4* nb_param; const unsigned int* excl; const int* exc_atoms; const float4* exc_par;
    const int4* unit_atoms; const unsigned char* unit_type; const float* shake_dist; settle_const sc; float tol;
    const float* invmass; const int64_t* labels; const double* beta; int r_begin; uint64_t seed; const unsigned int* noise_id;
    float inv_total_mass; unsigned int* shake_stat;
    listed_tables L; int n_listed;
};

// one token of the step program on the registers of a unit
template <int TYPE, int NAT>
__device__ __forceinline__ void resident_mol_token(char tok, const resident_prog& prog, int o_index, long long gstep, const int* idx, const float* dist,
                                                   const settle_const& sc, float tol, const long long* F, int Fs, float kT, uint32_t rg, uint64_t seed,
                                                   unit_regs& S)
{
    if (tok == 'V') {
        unit_kick_add<NAT>(prog.hV, idx, F, Fs, S);
        constrain_v<TYPE, NAT>(sc, S.im, tol, S.v, S.x);
    } else if (tok == 'R') {
        unit_drift<TYPE, NAT>(prog.hR, dist, sc, tol, S);
    } else if (tok == 'O') {
        const uint64_t cnt = (uint64_t)gstep * (uint64_t)prog.nO + (uint64_t)o_index;
        unit_ou<TYPE, NAT>(prog.a, prog.b, kT, cnt, seed, rg, idx, sc, tol, S);
    }
}

#define RESIDENT_MOL_T 256
#define RESIDENT_MOL_MAX_ATOMS 64
__global__ __launch_bounds__(RESIDENT_MOL_T)
void resident_mol_kernel(resident_prog prog, resident_mol_sys S, float4* __restrict__ pos, float4* __restrict__ vel)
{
    __shared__ float4 s_pos[RESIDENT_MOL_T], s_par[RESIDENT_MOL_T];
    __shared__ long long s_F[3 * RESIDENT_MOL_T];
    __shared__ long long s_pm[RESIDENT_MOL_T / 64][3];
    constexpr int Fs = RESIDENT_MOL_T;
    const int tid = threadIdx.x, r = blockIdx.x, N = S.N;
    float4* P = pos + (size_t)r * S.Npad;
    float4* V = vel + (size_t)r * S.Npad;
    int4 a4 = make_int4(-1, -1, -1, -1);
    int type = UNIT_FREE;
    float dist[3] = { 0.f, 0.f, 0.f };
    if (tid < S.n_units) {
        a4 = S.unit_atoms[tid]; type = (int)S.unit_type[tid];
        dist[0] = S.shake_dist[tid * 3]; dist[1] = S.shake_dist[tid * 3 + 1]; dist[2] = S.shake_dist[tid * 3 + 2];
    }
    const bool active = a4.x >= 0;
    if (!active) type = UNIT_FREE;
    const int idx[4] = { a4.x, a4.y, a4.z, a4.w };
    unit_regs U;
    U.have_cm = 0; U.shake_it = 0; U.heat = 0.f; U.shadow = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        U.x[k] = f3(0, 0, 0); U.v[k] = f3(0, 0, 0); U.im[k] = 0.f;
        if (idx[k] >= 0) {
            const float4 p = P[idx[k]], w = V[idx[k]];
            U.x[k] = f3(p.x, p.y, p.z); U.v[k] = f3(w.x, w.y, w.z); U.im[k] = S.invmass[idx[k]];
        }
    }
    s_par[tid] = tid < N ? S.nb_param[tid] : make_float4(0.f, 0.f, 0.f, 0.f);
    s_pos[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float kT = frcp((float)S.beta[S.labels[S.r_begin + r]]);
    const uint32_t rg = S.noise_id ? S.noise_id[r] : (uint32_t)(S.r_begin + r);
    bool forces_valid = false;
    __syncthreads();

    auto evaluate = [&]() {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (idx[k] >= 0) {
                s_pos[idx[k]] = make_float4(U.x[k].x, U.x[k].y, U.x[k].z, 0.f);
                s_F[idx[k]] = 0; s_F[Fs + idx[k]] = 0; s_F[2 * Fs + idx[k]] = 0;
            }
        }
        __syncthreads();
        if (tid < N) {
            const float4 xi = s_pos[tid], pi = s_par[tid];
            float fx = 0.f, fy = 0.f, fz = 0.f;
            double e = 0.0;
            const unsigned int* mrow = S.excl + (size_t)tid * S.words;
            for (int j0 = 0; j0 < N; j0 += 32) {
                const unsigned int m = mrow[j0 >> 5];
                const int jn = min(32, N - j0);
                for (int k = 0; k < jn; ++k) {
                    const int j = j0 + k;
                    if (j == tid || ((m >> k) & 1u)) continue;
                    nocutoff_pair<false>(xi, pi, s_pos[j], s_par[j], fx, fy, fz, e);
                }
            }
            add_force(s_F, Fs, tid, fx, fy, fz);
        }
        for (int t = tid; t < S.n_exc; t += RESIDENT_MOL_T) {
            const int i = S.exc_atoms[2 * t], j = S.exc_atoms[2 * t + 1];
            const float4 par = S.exc_par[t];
            const float3 d = sub3(ld3(s_pos, j), ld3(s_pos, i));
            double e = 0.0;
            const float fr = nocutoff_exception<false>(par, d, e);
            add_force(s_F, Fs, i, fr * d.x, fr * d.y, fr * d.z);
            add_force(s_F, Fs, j, -fr * d.x, -fr * d.y, -fr * d.z);
        }
        // (every lane of a wavefront takes part in listed_forces_body's reduction over the lanes of one atom)
        for (int base = 0; base < S.n_listed; base += RESIDENT_MOL_T)
            listed_forces_body(S.L, Fs, s_pos, (const float*)nullptr, s_F, base + tid, 0);
        __syncthreads();
        forces_valid = true;
    };

    for (int s = 0; s < prog.n_steps; ++s) {
        const long long gstep = prog.gstep0 + s;
        if (prog.cmm_frequency > 0 && ((prog.first_step + s) % prog.cmm_frequency) == 0) {
            // CMMotionRemover at the top of a step (integrators.py:1313): the sum of the chain kernel -- fp32 over a unit's atoms and the
            // units of a wavefront, then fixed point
            float3 pm = f3(0, 0, 0);
            if (active) {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (idx[k] >= 0) pm = pm + U.v[k] * frcp(U.im[k]);
            }
            for (int off = 32; off > 0; off >>= 1) { pm.x += __shfl_xor(pm.x, off); pm.y += __shfl_xor(pm.y, off); pm.z += __shfl_xor(pm.z, off); }
            if ((tid & 63) == 0) {
                long long* w = s_pm[tid >> 6];
                w[0] = (long long)((double)pm.x * 4294967296.0); w[1] = (long long)((double)pm.y * 4294967296.0); w[2] = (long long)((double)pm.z * 4294967296.0);
            }
            __syncthreads();
            long long tot[3] = { 0, 0, 0 };
            for (int w = 0; w < RESIDENT_MOL_T / 64; ++w) { tot[0] += s_pm[w][0]; tot[1] += s_pm[w][1]; tot[2] += s_pm[w][2]; }
            __syncthreads();
            const float sx = (float)tot[0] * FIXED_TO_F32 * S.inv_total_mass;
            const float sy = (float)tot[1] * FIXED_TO_F32 * S.inv_total_mass;
            const float sz = (float)tot[2] * FIXED_TO_F32 * S.inv_total_mass;
#pragma unroll
            for (int k = 0; k < 4; ++k) { U.v[k].x -= sx; U.v[k].y -= sy; U.v[k].z -= sz; }
        }
        int o_index = 0;
        for (int t = 0; t < prog.n; ++t) {
            // (the token from six registers loaded with the kernel arguments, the O counter kept here: a dynamic index into the argument
            //  arrays is a scalar memory load per token on a path that is all latency, see prog_tok)
            const char tok = prog_tok(prog, t);
            if (tok == 'V' && !forces_valid) evaluate();
            if (tok == 'R') forces_valid = false;
            const int o_now = o_index;
            if (tok == 'O') ++o_index;
            if (active) {
#define RUN(TY, NA) resident_mol_token<TY, NA>(tok, prog, o_now, gstep, idx, dist, S.sc, S.tol, s_F, Fs, kT, rg, S.seed, U)
                UNIT_LADDER(type, a4, RUN);
#undef RUN
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (idx[k] >= 0) {
            P[idx[k]] = make_float4(U.x[k].x, U.x[k].y, U.x[k].z, 0.f);
            V[idx[k]] = make_float4(U.v[k].x, U.v[k].y, U.v[k].z, 0.f);
        }
    }
    if (type == UNIT_SHAKE && U.shake_it > 0 &&
        (unsigned int)U.shake_it > __hip_atomic_load(S.shake_stat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(S.shake_stat, (unsigned int)U.shake_it);
}

// the small-molecule kernel
int remd_run_steps_resident_mol(remd_ctx* h, const std::vector<char>& tokens, int nV, int nR, int nO,
                                int64_t iteration, int64_t first_step, int n_steps)
{
    if (!resident_takes_request(h, tokens, n_steps)) return 0;
    if (!h->nocutoff || h->gbsa || h->n_regions > 0 || h->nb_method != REMD_NB_NONE || h->n_ext > 0 || h->n_restraints > 0 || h->n_custom > 0) return 0;
    const unit_tables& ut = remd_table_of(h->units);
    if (h->N > RESIDENT_MOL_MAX_ATOMS || ut.n_units > RESIDENT_MOL_T || ut.n_units < 1) return 0;
    resident_mol_sys S{};
    S.N = h->N; S.Npad = h->Npad; S.n_units = ut.n_units;
    if (remd_nocutoff_info(h, &S.nb_param, &S.excl, &S.words, &S.n_exc, &S.exc_atoms, &S.exc_par)) return 0;
    S.unit_atoms = ut.d_atoms; S.unit_type = ut.d_type; S.shake_dist = ut.d_dist; S.sc = ut.sc;
    S.tol = remd_constraint_tol(h);
    S.invmass = h->d_invmass; S.labels = h->d_labels; S.beta = h->d_beta; S.r_begin = h->r_begin; S.seed = h->seed; S.noise_id = h->d_noise_id;
    S.inv_total_mass = (float)(h->total_mass > 0 ? 1.0 / h->total_mass : 0.0);
    S.shake_stat = h->d_sync + 3;
    listed_tables L{};
    L.n_bonds = h->n_bonds; L.n_angles = h->n_angles; L.n_torsions = h->n_torsions;
    L.bond_atoms = h->d_bond_atoms; L.bond_params = h->d_bond_params;
    L.angle_atoms = h->d_angle_atoms; L.angle_params = h->d_angle_params;
    L.torsion_atoms = h->d_torsion_atoms; L.torsion_params = h->d_torsion_params;
    S.n_listed = L.n_bonds + L.n_angles + L.n_torsions;
    if (S.n_listed > 0 && h->d_aterm && h->n_aterm > 0) { L.aterm = h->d_aterm; L.n_aterm = h->n_aterm; S.n_listed = h->n_aterm; }
    S.L = L;
    const resident_prog prog = resident_program(h, tokens, nV, nR, nO, iteration, first_step, n_steps);
    remd_launch_join_wait(h);
    remd_prof_scope ps(h, "resident_md");
    hipLaunchKernelGGL(resident_mol_kernel, dim3(h->R), dim3(RESIDENT_MOL_T), 0, h->stream, prog, S, h->d_pos, h->d_vel);
    REMD_CHECK(h, hipGetLastError());
    h->forces_valid = false; h->force_zeroed = false;
    return 1;
}
