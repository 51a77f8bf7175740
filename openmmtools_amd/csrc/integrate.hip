// Langevin splitting integrator (gfx950): the chain kernel that runs the V / R / O substeps between two force evaluations and its
// host step loop, the Maxwell-Boltzmann velocity draw, kinetic-energy reduction, CM-motion removal, heat / shadow work and
// Metropolization.  The arithmetic of one constraint unit is in constraint_units.h (shared with resident.hip and minimize.hip).
//
// Reference semantics (restated; the substeps: constraint_units.h):
//   openmmtools/mcmc.py:710-711           setVelocitiesToTemperature (+ velocity constraints)
//   openmmtools/integrators.py:1313       addUpdateContextState (CMMotionRemover acts here, once per step)
//
// Design: one thread owns one *constraint unit* (a rigid water, an X-H cluster, or a free atom), keeps its <= 4 atoms' x and v in
// registers and runs the whole chain of substeps between two force evaluations without touching HBM in between.  All replicas of
// the rank are covered by one launch (blockIdx.y = replica).
#include "constraint_units.h"
#include <set>

#define CHAIN_BIN_COLS 256       // mesh columns (nx) a chain workgroup can bin in its LDS counters

// One launch of the chain.  It holds the fields of a step_prog (constraint_units.h) -- n, tok, o_index, hV, hR, a, b, nO: what prog_tok
// and remd_step_prog_fill use -- under the same names but not as a base: the chain kernel's instruction stream depends on where they
// sit among its arguments.
struct chain_prog {
    int n;                 // tokens in this chain
    char tok[MAX_TOK];     // 'V','R','O','C' (C = subtract centre-of-mass velocity)
    int o_index[MAX_TOK];  // for 'O': index of this O inside the step program
    long long step[MAX_TOK]; // global step index of each token (a chain may hold tokens left pending by the previous step)
    float hV, hR;          // dt/n_V, dt/n_R
    float hVg[4];          // multiple-time-step splittings: dt / (V tokens of force group g); tokens '0'..'3'
    const long long* Fg[4]; // forces of force group g ([R][3][Npad] fixed point, like the all-forces accumulator)
    float a, b; int nO;    // OU coefficients, O substeps per step
    int accumulate_momentum;  // after the chain, add sum(m v) into cmm buffer cmm_w
    int cmm_w, cmm_r;         // double-buffered momentum accumulators: 'C' reads cmm_r and clears the other one
    int zero_force;           // the chain ends with stale forces (an R after its last V): clear them for the next evaluation
    int m_buf;                // token 'M' (inside a chain): every workgroup of the replica publishes its partial sum(m v) as epoch-tagged 64-bit
    unsigned int m_epoch;     // words (m_epoch-th exchange of this handle, d_chain_sync) and reads its siblings': the 'C' behind it has the sum
    int measure;              // bit 0: heat (kinetic-energy change of the O substeps), bit 1: kinetic part of the shadow work (V, R substeps)
};

// the whole chain of substeps for one constraint unit, everything in registers
template <int TYPE, int NAT>
__device__ __forceinline__ float3 run_unit(const chain_prog& prog, const int* idx, const float* dist, const settle_const& sc,
                                          float tol, int Npad, float4* __restrict__ P, float4* __restrict__ V,
                                          const long long* F, long long* Fw, float kT, uint32_t rg, uint64_t seed,
                                          const long long* __restrict__ cmm_r, float inv_total_mass, const remd_chain_bins& bins, int r,
                                          unit_regs& S, int t0, int t1, bool first, bool last,
                                          float4* __restrict__ Xold, float4* __restrict__ Vold)
{
    float3 (&x)[4] = S.x; float3 (&v)[4] = S.v;
    float (&im)[4] = S.im;
    // kinetic energy of this unit's atoms (integrators.py:1141: 0.5 m v^2 summed over the degrees of freedom)
    auto unit_ke = [&]() { float ke = 0.f;
#pragma unroll
        for (int k = 0; k < NAT; ++k) ke += 0.5f * dot3(v[k], v[k]) * frcp(im[k]);
        return ke; };
    if (first) {
        S.heat = 0.f; S.shadow = 0.f;
#ifdef CHAIN_STAMPS
        if (S.stamps) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long now = wall_clock64(); atomicAdd(&S.stamps[1 + 21], now - S.t_last); S.t_last = now; }
#endif
    }
    for (int t = t0; t < t1; ++t) {
        const char tok = prog_tok(prog, t);
        const bool is_v = tok == 'V' || (tok >= '0' && tok <= '3');
        const float ke0 = ((prog.measure & 1) && tok == 'O') || ((prog.measure & 2) && (is_v || tok == 'R')) ? unit_ke() : 0.f;
        if (tok == '{') {
            // Metropolization starts: remember x and v (integrators.py:1539-1542)
#pragma unroll
            for (int k = 0; k < NAT; ++k) {
                Xold[idx[k]] = make_float4(x[k].x, x[k].y, x[k].z, 0.f);
                Vold[idx[k]] = make_float4(v[k].x, v[k].y, v[k].z, 0.f);
            }
        } else if (tok == 'V' || (tok >= '0' && tok <= '3')) {
            // all forces, or the forces of one force group with that group's share of the time step (integrators.py:1437-1440)
            const long long* Ft = tok == 'V' ? F : prog.Fg[tok - '0'] + (size_t)r * 3 * Npad;
            const float hv = tok == 'V' ? prog.hV : prog.hVg[tok - '0'];
            unit_kick_add<NAT>(hv, idx, Ft, Npad, S);
#ifdef CHAIN_STAMPS
            if (S.stamps && t == 0) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long now = wall_clock64(); atomicAdd(&S.stamps[1 + 22], now - S.t_last); S.t_last = now; }
#endif
            constrain_v<TYPE, NAT>(sc, im, tol, v, x);
        } else if (tok == 'R') {
            unit_drift<TYPE, NAT>(prog.hR, dist, sc, tol, S);
        } else if (tok == 'O') {
            const uint64_t cnt = (uint64_t)prog.step[t] * (uint64_t)prog.nO + (uint64_t)prog.o_index[t];
            unit_ou<TYPE, NAT>(prog.a, prog.b, kT, cnt, seed, rg, idx, sc, tol, S);
        } else if (tok == 'C') {
            // CMMotionRemover: v -= P/M with P accumulated by the previous chain or by the 'M' token in front (read at the
            // coherence point: other workgroups added to it by atomics during this launch)
            float sx, sy, sz;
            if (S.have_cm) { sx = S.cmx; sy = S.cmy; sz = S.cmz; }
            else {
                sx = (float)__hip_atomic_load(&cmm_r[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * FIXED_TO_F32 * inv_total_mass;
                sy = (float)__hip_atomic_load(&cmm_r[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * FIXED_TO_F32 * inv_total_mass;
                sz = (float)__hip_atomic_load(&cmm_r[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * FIXED_TO_F32 * inv_total_mass;
            }
#pragma unroll
            for (int k = 0; k < NAT; ++k) { v[k].x -= sx; v[k].y -= sy; v[k].z -= sz; }
        }
#ifdef CHAIN_STAMPS
        if (S.stamps) { const unsigned long long now = wall_clock64(); atomicAdd(&S.stamps[1 + min(t, 33)], now - S.t_last); S.t_last = now; }
#endif
        if ((prog.measure & 1) && tok == 'O') S.heat += unit_ke() - ke0;                           // :1448-1460
        if ((prog.measure & 2) && (is_v || tok == 'R')) S.shadow += unit_ke() - ke0;                // :1409-1446 (kinetic part)
    }
    float3 mom = f3(0, 0, 0);
    if (!last) return mom;
#pragma unroll
    for (int k = 0; k < NAT; ++k) {
        P[idx[k]] = make_float4(x[k].x, x[k].y, x[k].z, 0.f);
        V[idx[k]] = make_float4(v[k].x, v[k].y, v[k].z, 0.f);
        mom = mom + v[k] * frcp(im[k]);
        if (prog.zero_force) { Fw[idx[k]] = 0; Fw[Npad + idx[k]] = 0; Fw[2 * Npad + idx[k]] = 0; }
        if (bins.count) {
            // these positions are final for the force evaluation that follows: bin the atom by its PME mesh column here, so
            // that no binning launch sits between the integrator and the spreading pass (the order inside a bin is
            // irrelevant: charges and forces are fixed-point sums)
            float u; int kx;
            remd_pme_scaled1(x[k].x, bins.box[4 * r], bins.nx, u, kx);
            if (kx >= bins.nx) kx -= bins.nx;
            const int slot = atomicAdd(&bins.count[(size_t)r * bins.nx + kx], 1);
            if (slot < bins.cap) {
                const size_t e = ((size_t)r * bins.nx + kx) * bins.cap + slot;
                bins.atoms[e] = make_float4(x[k].x, x[k].y, x[k].z, __int_as_float(idx[k]));
                if (bins.q) bins.q[e] = bins.param[idx[k]].x;        // (state-independent charges only, see remd_pme_chain_bins)
            } else atomicCAS(bins.err, 0u, 2u);
        }
#ifdef CHAIN_STAMPS
        if (S.stamps) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long now = wall_clock64(); atomicAdd(&S.stamps[1 + 24 + k], now - S.t_last); S.t_last = now; }
#endif
    }
#ifdef CHAIN_STAMPS
    if (S.stamps) { const unsigned long long now = wall_clock64(); atomicAdd(&S.stamps[35], now - S.t_last); S.t_last = now; }
#endif
    return mom;
}

__device__ __forceinline__ void integrate_chain_body(chain_prog prog, int n_units, const int4* __restrict__ unit_atoms,
                            const unsigned char* __restrict__ unit_type, const float* __restrict__ shake_dist,
                            settle_const sc, float tol,
                            int Npad, float4* __restrict__ pos, float4* __restrict__ vel,
                            long long* force, const float* __restrict__ invmass,
                            const int64_t* __restrict__ labels, const double* __restrict__ beta,
                            int r_begin, uint64_t seed, long long* __restrict__ cmm, float inv_total_mass,
                            unsigned int* join_flag, unsigned int join_seq, remd_chain_bins bins,
                            unsigned long long* chain_slots, unsigned int* chain_sync_err,
                            unsigned long long* own_time, long long* __restrict__ work, float4* __restrict__ xold, float4* __restrict__ vold,
                            remd_fold_args fold, const unsigned int* __restrict__ noise_id)
{
    // What does not depend on the forces travels while this workgroup waits for them (or, when they are complete already, all at once
    // instead of table -> type -> distances and label -> beta one round trip after the other): the unit table, positions, velocities,
    // masses, the state's temperature.  Positions and velocities are written by the previous chain launch of this stream only.
    const int uidx = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    // (written out, not load_unit_row / load_unit_atoms: through the shared loaders this kernel, at its register limit, is allocated
    //  differently -- 110 -> 134 AGPRs)
    int4 a4 = make_int4(-1, -1, -1, -1);
    int type = UNIT_FREE;
    float dist[3] = { 0.f, 0.f, 0.f };
    float kT = 0.f;
    uint32_t rg = 0u;
    unit_regs S;
    S.have_cm = 0; S.shake_it = 0;
    {
        if (uidx < n_units) {
            a4 = unit_atoms[uidx]; type = (int)unit_type[uidx];
            dist[0] = shake_dist[uidx * 3]; dist[1] = shake_dist[uidx * 3 + 1]; dist[2] = shake_dist[uidx * 3 + 2];
        }
        kT = frcp((float)beta[labels[r_begin + r]]);       // fp32 state: 1 ulp of kT is below its own rounding
        rg = noise_id ? noise_id[r] : (uint32_t)(r_begin + r);
        const int e_idx[4] = { a4.x, a4.y, a4.z, a4.w };
        const float4* Pe = pos + (size_t)r * Npad;
        const float4* Ve = vel + (size_t)r * Npad;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e_idx[k] >= 0) {
                const float4 p = Pe[e_idx[k]], w = Ve[e_idx[k]];
                S.x[k] = f3(p.x, p.y, p.z); S.v[k] = f3(w.x, w.y, w.z); S.im[k] = invmass[e_idx[k]];
            }
        }
    }
    if (fold.done) {
        // remd_fold_args: wait until every workgroup of the direct-space stream's last launch has counted itself done (their force
        // atomics are complete by then)
        // one counter per replica, each on its own cache line (done[16 r]): a replica's chain workgroups need that replica's forces
        // only, and a few hundred arrivals on ONE address serialise at the memory side (~35 ns each: profiles/r04_p_*)
        if (threadIdx.x == 0) {
            const unsigned int* word = fold.done + 16 * blockIdx.y;
            long long n = 0;
            while ((int)(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - fold.target) < 0) {
                // (a fault is already raised -- this propagation is run again whatever happens from here: do not wait a second time;
                // without this every step behind a poll that ran out waits for its own time-out, seconds each; looked at every 256th poll
                // only, from the 256th on: a wait of ordinary length never pays for the extra load)
                if ((n & 255) == 255 && __hip_atomic_load(chain_sync_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
                __builtin_amdgcn_s_sleep(2);
                if (++n > (1ll << 25)) { atomicCAS(chain_sync_err, 0u, 1u); break; }
            }
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    if (join_flag) {
        // the forces of the direct-space stream: poll its "done" flag here instead of behind a cross-stream event (remd_ctx::d_sync)
        if (threadIdx.x == 0) {
            long long n = 0;
            while ((int)(__hip_atomic_load(join_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - join_seq) < 0) {
                if ((n & 255) == 255 && __hip_atomic_load(join_flag + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;   // (as above)
                __builtin_amdgcn_s_sleep(2);
                if (++n > (1ll << 25)) { atomicCAS(join_flag + 1, 0u, 1u); break; }
            }
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    // profiling: this launch's OWN time, from "forces complete" seen to the end, for workgroup (0, 0) (the launch duration a
    // profiler reports also holds the wait for the direct-space stream in the prologue)
    const unsigned long long own_t0 = own_time ? wall_clock64() : 0ull;
    float3 mom = f3(0, 0, 0);
    const int cmm_r_eff = prog.cmm_r, cmm_w_eff = prog.cmm_w;
    if (uidx == 0 && cmm_r_eff >= 0) {
        // this chain consumes accumulator cmm_r: clear the OTHER buffer (its sum was consumed one step ago)
        long long* o = cmm + ((size_t)(1 - cmm_r_eff) * gridDim.y + r) * 4;
        o[0] = 0; o[1] = 0; o[2] = 0;
    }
    const bool active = a4.x >= 0;                              // padding units do nothing (but take part in the 'M' barrier)
    if (!active) type = UNIT_FREE;
    const int idx[4] = { a4.x, a4.y, a4.z, a4.w };
    float4* P = pos + (size_t)r * Npad;
    float4* V = vel + (size_t)r * Npad;
    const long long* F = force + (size_t)r * 3 * Npad;
    long long* Fw = force + (size_t)r * 3 * Npad;
    const long long* cr = cmm + ((size_t)max(cmm_r_eff, 0) * gridDim.y + r) * 4;
#ifdef CHAIN_STAMPS
    S.stamps = (own_time && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) ? own_time + 2 : nullptr;
    S.t_last = own_t0;
#endif
    // mesh-column bins: by the workgroup (below, behind the token program) when the columns fit its LDS counters, else atom by atom
    // at the end of run_unit
    const bool wg_bins = bins.count != nullptr && bins.nx <= CHAIN_BIN_COLS;
    remd_chain_bins unit_bins = bins;
    if (wg_bins) unit_bins.count = nullptr;
#ifdef CHAIN_STAMPS
    if (S.stamps) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long now = wall_clock64(); atomicAdd(&S.stamps[1 + 20], now - S.t_last); S.t_last = now; }
#endif
    // segments of the token program, split at 'M' (momentum sum + barrier over the replica's workgroups)
    for (int t0 = 0;;) {
        int t1 = t0;
        while (t1 < prog.n && prog_tok(prog, t1) != 'M') ++t1;
        const bool first = t0 == 0, last = t1 == prog.n;
        if (active) {
#define RUN(TY, NA) mom = run_unit<TY, NA>(prog, idx, dist, sc, tol, Npad, P, V, F, Fw, kT, rg, seed, cr, inv_total_mass, unit_bins, r, S, t0, t1, first, last, xold ? xold + (size_t)r * Npad : nullptr, vold ? vold + (size_t)r * Npad : nullptr)
            UNIT_LADDER(type, a4, RUN);
#undef RUN
        }
        if (last) break;
        {
            // 'M': sum(m v) of the velocities as they are now, over all workgroups of this replica (all of them are resident: the launcher
            // checks the grid size).  One exchange through device memory: a workgroup publishes its three fixed-point partial sums as
            // 64-bit words that carry the epoch of this barrier in their low 16 bits (48-bit payload), in the epoch's parity half of
            // chain_slots [2][replica][workgroup][3]; every workgroup then reads all words of its replica, spinning on a word until its
            // tag is this epoch's.  A word is rewritten two epochs later, which its writer cannot reach before every reader has published
            // the epoch in between, i.e. is done with this one.  (Before: atomics into one accumulator + an arrival counter + a read-back
            // = three dependent round trips, 5.1 us of the headline step's 27 us chain; the sum is the same integer.)
            __shared__ long long s_pm[4][3];
            __shared__ unsigned long long s_tot[3];
            float3 pm = f3(0, 0, 0);
            if (active) {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (idx[k] >= 0) pm = pm + S.v[k] * frcp(S.im[k]);
            }
            for (int off = 32; off > 0; off >>= 1) {
                pm.x += __shfl_xor(pm.x, off); pm.y += __shfl_xor(pm.y, off); pm.z += __shfl_xor(pm.z, off);
            }
            if ((threadIdx.x & 63) == 0) {
                long long* w = s_pm[threadIdx.x >> 6];
                w[0] = (long long)((double)pm.x * 4294967296.0); w[1] = (long long)((double)pm.y * 4294967296.0); w[2] = (long long)((double)pm.z * 4294967296.0);
            }
            if (threadIdx.x < 3) s_tot[threadIdx.x] = 0ull;
            __syncthreads();
            const unsigned long long tag = (unsigned long long)(prog.m_epoch & 0xffffu);
            unsigned long long* slots = chain_slots + ((size_t)(prog.m_epoch & 1u) * gridDim.y + r) * gridDim.x * 3;
            if (threadIdx.x < 3) {
                const long long t = s_pm[0][threadIdx.x] + s_pm[1][threadIdx.x] + s_pm[2][threadIdx.x] + s_pm[3][threadIdx.x];
                if (t >= (1ll << 46) || t < -(1ll << 46)) atomicCAS(chain_sync_err, 0u, 7u);       // (a fault of its own: the host then sums with two launches, the polled waits stay)
                __hip_atomic_store(&slots[blockIdx.x * 3 + threadIdx.x], ((unsigned long long)t << 16) | tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const int n_words = 3 * (int)gridDim.x;
            if (threadIdx.x < 255 && (int)threadIdx.x < n_words) {
                long long part = 0;
                for (int q = threadIdx.x; q < n_words; q += 255) {          // (255 = 0 mod 3: a thread stays on one component)
                    unsigned long long w;
                    long long n = 0;
                    while (((w = __hip_atomic_load(&slots[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0xffffull) != tag) {
                        if ((n & 255) == 255 && __hip_atomic_load(chain_sync_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;   // (as in the prologue)
                        __builtin_amdgcn_s_sleep(1);
                        if (++n > (1ll << 25)) { atomicCAS(chain_sync_err, 0u, 3u); break; }
                    }
                    part += (long long)w >> 16;
                }
                atomicAdd(&s_tot[threadIdx.x % 3], (unsigned long long)part);
            }
            __syncthreads();
            S.cmx = (float)(long long)s_tot[0] * FIXED_TO_F32 * inv_total_mass;
            S.cmy = (float)(long long)s_tot[1] * FIXED_TO_F32 * inv_total_mass;
            S.cmz = (float)(long long)s_tot[2] * FIXED_TO_F32 * inv_total_mass;
            S.have_cm = 1;
            __syncthreads();                                    // (s_pm / s_tot may be written again by a second 'M' of this launch)
#ifdef CHAIN_STAMPS
            if (S.stamps) { const unsigned long long now = wall_clock64(); atomicAdd(&S.stamps[1 + min(t1, 33)], now - S.t_last); S.t_last = now; }
#endif
        }
        t0 = t1 + 1;
    }
    if (wg_bins) {
        // The final positions of this workgroup's atoms, binned by PME mesh column for the spreading pass that follows (the order inside
        // a bin is irrelevant: charges and forces are fixed-point sums).  One atomic with a returned slot per ATOM made the end of the chain
        // three dependent rounds per unit (each behind the stores issued before it: one in-order counter) on ~35 atoms per counter;
        // here the atoms take ranks in LDS counters, the workgroup reserves one range per occupied column with ONE returning atomic,
        // and every atom stores at base + rank.
        __shared__ int s_bin_cnt[CHAIN_BIN_COLS], s_bin_base[CHAIN_BIN_COLS];
        for (int c = threadIdx.x; c < bins.nx; c += blockDim.x) s_bin_cnt[c] = 0;
        __syncthreads();
        int col[4] = { 0, 0, 0, 0 }, rank[4] = { 0, 0, 0, 0 };
        if (active) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (idx[k] >= 0) {
                    float u; int kx;
                    remd_pme_scaled1(S.x[k].x, bins.box[4 * r], bins.nx, u, kx);
                    if (kx >= bins.nx) kx -= bins.nx;
                    col[k] = kx; rank[k] = atomicAdd(&s_bin_cnt[kx], 1);
                }
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < bins.nx; c += blockDim.x) {
            const int n = s_bin_cnt[c];
            if (n > 0) s_bin_base[c] = atomicAdd(&bins.count[(size_t)r * bins.nx + c], n);
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (idx[k] >= 0) {
                    const int slot = s_bin_base[col[k]] + rank[k];
                    if (slot < bins.cap) {
                        const size_t e = ((size_t)r * bins.nx + col[k]) * bins.cap + slot;
                        bins.atoms[e] = make_float4(S.x[k].x, S.x[k].y, S.x[k].z, __int_as_float(idx[k]));
                        if (bins.q) bins.q[e] = bins.param[idx[k]].x;        // (state-independent charges only, see remd_pme_chain_bins)
                    } else atomicCAS(bins.err, 0u, 2u);
                }
            }
        }
#ifdef CHAIN_STAMPS
        if (S.stamps) { const unsigned long long now = wall_clock64(); atomicAdd(&S.stamps[1 + 27], now - S.t_last); S.t_last = now; }
#endif
    }
    if (prog.accumulate_momentum) {
        // wavefront shuffle reduction, one fixed-point atomic per wave (integer => order-independent sum)
        for (int off = 32; off > 0; off >>= 1) {
            mom.x += __shfl_xor(mom.x, off); mom.y += __shfl_xor(mom.y, off); mom.z += __shfl_xor(mom.z, off);
        }
        if ((threadIdx.x & 63) == 0) {
            unsigned long long* c = reinterpret_cast<unsigned long long*>(cmm + ((size_t)cmm_w_eff * gridDim.y + r) * 4);
            atomicAdd(&c[0], (unsigned long long)(long long)((double)mom.x * 4294967296.0));
            atomicAdd(&c[1], (unsigned long long)(long long)((double)mom.y * 4294967296.0));
            atomicAdd(&c[2], (unsigned long long)(long long)((double)mom.z * 4294967296.0));
        }
    }
    if (prog.measure && work) {
        // heat / kinetic shadow work of this launch: wavefront sums, one fixed-point atomic per wave (order-independent)
        float hq = active ? S.heat : 0.f, sw = active ? S.shadow : 0.f;
        for (int off = 32; off > 0; off >>= 1) { hq += __shfl_xor(hq, off); sw += __shfl_xor(sw, off); }
        if ((threadIdx.x & 63) == 0) {
            unsigned long long* w = reinterpret_cast<unsigned long long*>(work + 4 * (size_t)r);
            if (prog.measure & 1) atomicAdd(&w[0], (unsigned long long)(long long)((double)hq * 16777216.0));
            if (prog.measure & 2) atomicAdd(&w[1], (unsigned long long)(long long)((double)sw * 16777216.0));
        }
    }
    // most Newton updates any X-H position solve of this handle has needed (remd_get_constraint_stats): d_sync[3], next to the fault
    // word.  The word only ever grows and stops changing after the first steps, so a lane looks before it writes (no atomic otherwise).
    if (type == UNIT_SHAKE && S.shake_it > 0 &&
        (unsigned int)S.shake_it > __hip_atomic_load(chain_sync_err + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(chain_sync_err + 1, (unsigned int)S.shake_it);
    if (own_time && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        atomicAdd(&own_time[0], wall_clock64() - own_t0);
        atomicAdd(&own_time[1], 1ull);
    }
}

// The integrator's working set under the widest unit type is 256 VGPRs + AGPRs = one wavefront per SIMD, one workgroup per CU; a grid
// larger than the chip then runs in rounds (DHFR x 16: 512 workgroups).  (The body stays a function of its own: it works on copies of
// the arguments, the kernel's parameters would be read in place -- another instruction stream.)
__global__ __launch_bounds__(256)
void integrate_chain_kernel(chain_prog prog, int n_units, const int4* __restrict__ unit_atoms, const unsigned char* __restrict__ unit_type,
                            const float* __restrict__ shake_dist, settle_const sc, float tol, int Npad, float4* __restrict__ pos,
                            float4* __restrict__ vel, long long* force, const float* __restrict__ invmass, const int64_t* __restrict__ labels,
                            const double* __restrict__ beta, int r_begin, uint64_t seed, long long* __restrict__ cmm, float inv_total_mass,
                            unsigned int* join_flag, unsigned int join_seq, remd_chain_bins bins, unsigned long long* chain_slots,
                            unsigned int* chain_sync_err, unsigned long long* own_time, long long* __restrict__ work, float4* __restrict__ xold,
                            float4* __restrict__ vold, remd_fold_args fold, const unsigned int* __restrict__ noise_id)
{
    integrate_chain_body(prog, n_units, unit_atoms, unit_type, shake_dist, sc, tol, Npad, pos, vel, force, invmass, labels, beta, r_begin, seed,
                         cmm, inv_total_mass, join_flag, join_seq, bins, chain_slots, chain_sync_err, own_time, work, xold, vold, fold, noise_id);
}

// Maxwell-Boltzmann velocities (mcmc.py:710-711): v = sqrt(kT/m) xi, then velocity constraints.
template <int TYPE, int NAT>
__device__ __forceinline__ void assign_unit(const int* idx, const settle_const& sc, float tol, const float4* __restrict__ P,
                                            float4* __restrict__ V, const float* __restrict__ invmass, float kT, uint32_t rg,
                                            uint64_t seed, int64_t iteration)
{
    float3 x[NAT], v[NAT];
    float im[NAT];
#pragma unroll
    for (int k = 0; k < NAT; ++k) {
        const float4 p = P[idx[k]];
        x[k] = f3(p.x, p.y, p.z);
        im[k] = invmass[idx[k]];
        const float3 xi = gaussian3(seed, REMD_STREAM_VELOCITY, (uint32_t)idx[k], rg, (uint64_t)iteration);
        const float sig = fsqrt(kT * im[k]);
        v[k] = xi * sig;
    }
    constrain_v<TYPE, NAT>(sc, im, tol, v, x);
#pragma unroll
    for (int k = 0; k < NAT; ++k) V[idx[k]] = make_float4(v[k].x, v[k].y, v[k].z, 0.f);
}

__global__ __launch_bounds__(256)
void assign_velocities_kernel(int n_units, const int4* __restrict__ unit_atoms,
                              const unsigned char* __restrict__ unit_type, settle_const sc, float tol,
                              int Npad, const float4* __restrict__ pos, float4* __restrict__ vel,
                              const float* __restrict__ invmass, const int64_t* __restrict__ labels,
                              const double* __restrict__ beta, int r_begin, uint64_t seed, int64_t iteration,
                              const unsigned int* __restrict__ noise_id)
{
    const int uidx = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (uidx >= n_units) return;
    const int4 a4 = unit_atoms[uidx];
    if (a4.x < 0) return;
    const int idx[4] = { a4.x, a4.y, a4.z, a4.w };
    const int type = unit_type[uidx];
    const float4* P = pos + (size_t)r * Npad;
    float4* V = vel + (size_t)r * Npad;
    const float kT = frcp((float)beta[labels[r_begin + r]]);       // fp32 state: 1 ulp of kT is below its own rounding
    const uint32_t rg = noise_id ? noise_id[r] : (uint32_t)(r_begin + r);
#define RUN(TY, NA) assign_unit<TY, NA>(idx, sc, tol, P, V, invmass, kT, rg, seed, iteration)
    UNIT_LADDER(type, a4, RUN);
#undef RUN
}

// KE = sum 1/2 m v^2 per replica: per-lane partial -> wave shuffle -> LDS -> one value per block,
// blocks of one replica are summed in fixed order by the last stage (deterministic).
__global__ __launch_bounds__(256)
void kinetic_energy_kernel(int N, int Npad, const float4* __restrict__ vel, const float* __restrict__ mass,
                           double* __restrict__ ke)
{
    __shared__ double s_part[4];
    const int r = blockIdx.x;
    const float4* V = vel + (size_t)r * Npad;
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const float4 v = V[i];
        acc += 0.5 * (double)mass[i] * ((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ke[r] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

__global__ void check_finite_kernel(int N, int Npad, const float4* __restrict__ pos, const float4* __restrict__ vel, int* __restrict__ nan_flag)
{
    const int r = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float4 p = pos[(size_t)r * Npad + i], v = vel[(size_t)r * Npad + i];
    const float s = p.x + p.y + p.z + v.x + v.y + v.z;
    if (!isfinite(s)) nan_flag[r] = 1;
}

// ---------------------------------------------------------------------------------------------
void remd_table_deleter::operator()(unit_tables* t) const { delete t; }

// The analytic water solve takes its centre of mass and ra / rb from ONE set of masses, the first water's: a water with others (D2O,
// 18-O) would get correct bond lengths around the wrong centre of mass.  Refused; remd_set_system asks before it changes the handle.
int remd_check_settle_masses(remd_ctx* h, const remd_system_desc* d)
{
    for (int s = 0; s < d->n_settle; ++s) {
        const int* a = d->settle_atoms + 3 * s;
        for (int k = 0; k < 3; ++k) if (a[k] < 0 || a[k] >= d->n_atoms) return remd_fail(h, -3, "bad SETTLE triple");
        for (int k = 0; k < 3; ++k)
            if (fabs(d->mass[a[k]] - d->mass[d->settle_atoms[k]]) > 1e-9)
                return remd_fail(h, -3, "remd_set_system: SETTLE waters must share one set of masses");
    }
    return 0;
}

int remd_build_constraints(remd_ctx* h, const remd_system_desc* d)
{
    const int N = d->n_atoms;
    { const int rc = remd_check_settle_masses(h, d); if (rc) return rc; }      // before the handle's tables are touched
    h->units.reset(new unit_tables());
    unit_tables& ut = *h->units;
    std::vector<char> used(N, 0);
    std::vector<int4> atoms; std::vector<unsigned char> type; std::vector<float> dist;
    for (int s = 0; s < d->n_settle; ++s) {
        const int* a = d->settle_atoms + 3 * s;
        atoms.push_back(make_int4(a[0], a[1], a[2], -1)); type.push_back(UNIT_SETTLE);
        dist.push_back(0); dist.push_back(0); dist.push_back(0);
        for (int k = 0; k < 3; ++k) { if (a[k] < 0 || a[k] >= N || used[a[k]]) return remd_fail(h, -3, "bad SETTLE triple"); used[a[k]] = 1; }
    }
    while (atoms.size() % 64) { atoms.push_back(make_int4(-1, -1, -1, -1)); type.push_back(UNIT_SETTLE); dist.push_back(0); dist.push_back(0); dist.push_back(0); }
    for (int s = 0; s < d->n_shake; ++s) {
        const int* a = d->shake_atoms + 4 * s;
        atoms.push_back(make_int4(a[0], a[1], a[2], a[3])); type.push_back(UNIT_SHAKE);
        for (int k = 0; k < 3; ++k) dist.push_back((float)d->shake_dist[3 * s + k]);
        for (int k = 0; k < 4; ++k) if (a[k] >= 0) { if (a[k] >= N || used[a[k]]) return remd_fail(h, -3, "bad SHAKE cluster"); used[a[k]] = 1; }
    }
    auto pad64 = [&](unsigned char ty) {
        // units of one kind fill whole wavefronts: no wave mixes SETTLE, SHAKE and free-atom code paths
        while (atoms.size() % 64) { atoms.push_back(make_int4(-1, -1, -1, -1)); type.push_back(ty); dist.push_back(0); dist.push_back(0); dist.push_back(0); }
    };
    pad64(UNIT_SHAKE);
    // unconstrained atoms: FOUR to a unit while they last, the remainder one each (a unit = a thread; on DHFR -- 7023 waters, 790 X-H
    // clusters, 464 free atoms -- single-atom units made 8336 units = 33 workgroups per replica, and at one workgroup per CU (this
    // kernel's registers) 16 x 33 = 528 workgroups are THREE rounds of the chip; four to a unit: 7988 units = 32 workgroups, 512 = two rounds)
    {
        std::vector<int> fr;
        // (a massless particle -- a virtual site, virtual_sites.hip -- is in no unit: nothing that works on units moves or kicks it)
        for (int i = 0; i < N; ++i) {
            if (d->mass[i] == 0.0) { if (used[i]) return remd_fail(h, -3, "a massless particle (virtual site) takes part in a constraint"); continue; }
            if (!used[i]) fr.push_back(i);
        }
        size_t q = 0;
        for (; q + 4 <= fr.size(); q += 4) {
            atoms.push_back(make_int4(fr[q], fr[q + 1], fr[q + 2], fr[q + 3])); type.push_back(UNIT_FREE);
            dist.push_back(0); dist.push_back(0); dist.push_back(0);
        }
        for (; q < fr.size(); ++q) {
            atoms.push_back(make_int4(fr[q], -1, -1, -1)); type.push_back(UNIT_FREE);
            dist.push_back(0); dist.push_back(0); dist.push_back(0);
        }
    }
    ut.n_units = (int)atoms.size();
    REMD_TRY(ut.d_atoms.upload(h, atoms));
    REMD_TRY(ut.d_type.upload(h, type));
    REMD_TRY(ut.d_dist.upload(h, dist));
    h->n_settle = d->n_settle; h->n_shake = d->n_shake;
    int n_con = 3 * d->n_settle;
    for (int s = 0; s < d->n_shake; ++s) for (int k = 1; k < 4; ++k) if (d->shake_atoms[4 * s + k] >= 0) n_con++;
    h->n_dof = 3 * (N - h->n_massless) - n_con - (d->cmm_frequency > 0 ? 3 : 0);
    if (d->n_settle > 0) {
        const int* a = d->settle_atoms;
        const double mO = d->mass[a[0]], mH = d->mass[a[1]];
        const double rc = 0.5 * d->settle_dHH;
        const double t = sqrt(d->settle_dOH * d->settle_dOH - rc * rc);
        const double ra = 2.0 * mH * t / (mO + 2.0 * mH);
        ut.sc.mO = (float)mO; ut.sc.mH = (float)mH; ut.sc.ra = (float)ra; ut.sc.rb = (float)(t - ra);
        ut.sc.rc = (float)rc; ut.sc.dOH = (float)d->settle_dOH; ut.sc.dHH = (float)d->settle_dHH;
    }
    return 0;
}

int remd_parse_splitting(remd_ctx* h, const char* splitting, std::vector<char>& tokens, int& nV, int& nR, int& nO, int* nVg)
{
    // integrators.py:1474-1537: space-separated, case-insensitive V/R/O tokens, Metropolization braces, and force-group
    // suffixes V0, V1, ...: with more than one distinct group the splitting is a multiple-time-step one, every V must name its
    // group (:1527-1529) and takes dt / (occurrences of that group) with that group's forces only (:1437-1438); with one group
    // (or none) every V uses all forces and dt / (number of V tokens) (:1440, :1535)
    tokens.clear(); nV = nR = nO = 0;
    std::string s(splitting ? splitting : "");
    std::vector<int> vgroup;             // per V token: group index or -1 (no suffix)
    size_t i = 0;
    while (i < s.size()) {
        while (i < s.size() && s[i] == ' ') ++i;
        if (i >= s.size()) break;
        size_t j = i; while (j < s.size() && s[j] != ' ') ++j;
        std::string tok = s.substr(i, j - i);
        for (auto& c : tok) c = (char)toupper(c);
        if (tok[0] == 'V' && tok.find_first_not_of("0123456789", 1) == std::string::npos) {
            int g = -1;
            if (tok.size() > 1) {
                if (tok.size() > 3) return remd_fail(h, -3, "force group of '" + tok + "' out of range");
                g = atoi(tok.c_str() + 1);
                if (g > 31) return remd_fail(h, -3, "OpenMM only allows up to 32 force groups (integrators.py:1346-1347)");
            }
            tokens.push_back('V'); vgroup.push_back(g); nV++;
        }
        else if (tok == "R") { tokens.push_back('R'); nR++; }
        else if (tok == "O") { tokens.push_back('O'); nO++; }
        else if (tok == "{" || tok == "}") tokens.push_back(tok[0]);      // Metropolization of the substeps in between (:1539-1557)
        else return remd_fail(h, -3, "unsupported splitting token '" + tok + "' (supported: V V<group> R O { })");
        i = j;
    }
    {
        std::set<int> groups;
        for (int g : vgroup) if (g >= 0) groups.insert(g);
        int counts[4] = {0, 0, 0, 0};
        if (groups.size() > 1) {
            if (!nVg) return remd_fail(h, -3, "multiple-time-step splittings are set with remd_set_integrator");
            size_t v = 0;
            for (auto& c : tokens) if (c == 'V') {
                const int g = vgroup[v++];
                if (g < 0) return remd_fail(h, -3, "a multiple-time-step splitting must name the force group of every V (integrators.py:1527-1529)");
                if (g > 3) return remd_fail(h, -3, "force groups above 3 are not supported in multiple-time-step splittings");
                c = (char)('0' + g); counts[g]++;
            }
        }
        if (nVg) for (int g = 0; g < 4; ++g) nVg[g] = counts[g];
    }
    if (tokens.empty()) return remd_fail(h, -3, "empty splitting string");
    if (nR == 0 || nV == 0) return remd_fail(h, -3, "splitting needs at least one R and one V (integrators.py:1376-1385)");
    int depth = 0;
    for (char c : tokens) {
        if (c == '{') { if (++depth > 1) return remd_fail(h, -3, "nested '{' in the splitting string"); }
        else if (c == '}') { if (--depth < 0) return remd_fail(h, -3, "'}' without '{' in the splitting string"); }
        else if (c == 'O' && depth > 0) return remd_fail(h, -3, "O substeps cannot be Metropolized (integrators.py:1387-1401)");
    }
    if (depth != 0) return remd_fail(h, -3, "'{' without '}' in the splitting string");
    return 0;
}

static void launch_chain(remd_ctx* h, const unit_tables& ut, const chain_prog& prog, bool bin_for_pme = false)
{
    // mesh-column bins from the chain's epilogue: in a handle that runs as ONE block (the binning launch would sit on the step's only
    // critical path); the blocks of a phased propagation bin with a launch of their own, which runs beside the other block's kernels while
    // the chain is the serial part of both (24 x alanine dipeptide: 17.5 -> 18.2 it/s; one block of 8 x CB7:B2: 13.2 -> 12.2 the other way;
    // profiles/r06_45).  REMD_PME_CHAINBIN=0 / 1 pins it (bit-identical either way: the order inside a bin is irrelevant).
    // (a block whose chain grid is several rounds of the chip -- 64 x DHFR: 2 048 workgroups -- keeps them too: there the epilogue is
    // amortised over the rounds and the binning launch is the dearer one, 3.38 -> 3.46 s per iteration of 128 x DHFR without this bound)
    const bool chain_bins = h->sw.pme_chainbin >= 0 ? h->sw.pme_chainbin != 0
                                                    : (h->parent == nullptr || (long long)((ut.n_units + 255) / 256) * h->R > 1024);
    const remd_chain_bins bins = (bin_for_pme && chain_bins) ? remd_pme_chain_bins(h) : remd_chain_bins();
    remd_prof_scope ps(h, "integrate_chain");
    dim3 grid((ut.n_units + 255) / 256, h->R);
    // (A two-per-CU compilation took a grid larger than the chip in one round (DHFR x 16: -1.3 % of the converged step), but its workgroups
    // held the WHOLE register file of their CUs while they polled for the forces in the prologue, and a direct-space stream that still had
    // workgroups to place then never got a slot: the poll ran out after seconds (end of round 5, 128 alanine replicas = 384 workgroups).
    // Removed; one workgroup per CU leaves 160 registers per lane for the kernels the chain waits for.)
    const remd_handover::wait_t join = h->next.take_wait();      // the evaluation in front left it for this launch
    hipLaunchKernelGGL(integrate_chain_kernel, grid, dim3(256), 0, h->stream, prog, ut.n_units, ut.d_atoms, ut.d_type,
                       ut.d_dist, ut.sc, remd_constraint_tol(h), h->Npad, h->d_pos, h->d_vel, h->d_force,
                       h->d_invmass, h->d_labels, h->d_beta, h->r_begin, h->seed, h->d_cmm,
                       (float)(h->total_mass > 0 ? 1.0 / h->total_mass : 0.0),
                       join.seq ? h->d_sync + 1 : (unsigned int*)nullptr, join.seq, bins, h->d_chain_sync, h->d_sync + 2,
                       (h->profiling == 2 || (h->profiling == 1 && h->prof_filter.find("integrate_chain") != std::string::npos)) ? h->d_chain_own : (unsigned long long*)nullptr,
                       h->d_work, h->d_xold, h->d_vold, join.fold, h->d_noise_id);
    if (bins.count) h->next.cbins_ready = true;
}

// ---------------------------------------------------------------------------------------------------------------------
// Heat, shadow work and Metropolization (integrators.py:1175-1204, 1404-1460, 1539-1557).  The kinetic-energy changes of the
// substeps are summed inside the chain kernel (fixed point, per replica); the potential-energy change of an R substep needs the
// energy at the positions before and after it: remd_run_steps evaluates energies there (the evaluation behind an R also
// provides the forces of the V that follows, so a step of "V R O R V" costs two evaluations with energies instead of one without).
#define WORK_SCALE 16777216.0        // 2^24: 6e-8 kJ/mol
__global__ void work_pe_kernel(int R, const double* __restrict__ U, double* __restrict__ pe_prev, long long* __restrict__ work, int accumulate)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    if (accumulate) work[4 * r + 1] += (long long)((U[r] - pe_prev[r]) * WORK_SCALE);          // :1420-1423 (potential part)
    pe_prev[r] = U[r];
}
// '}' (:1544-1557): accept = step(exp(-shadow_work / kT) - uniform); trials++; on rejection x = xold, v = -vold; shadow_work = 0
__global__ void metropolis_kernel(int R, int r_begin, uint64_t seed, long long gstep, int brace, const int64_t* __restrict__ labels,
                                  const double* __restrict__ beta, long long* __restrict__ work, int* __restrict__ accept,
                                  const unsigned int* __restrict__ noise_id)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const double sw = (double)work[4 * r + 1] / WORK_SCALE;
    const philox4 w = remd_philox(seed, REMD_STREAM_METROPOLIS, (uint32_t)brace, noise_id ? noise_id[r] : (uint32_t)(r_begin + r), (uint64_t)gstep);
    const double u = remd_u53(w.w[2], w.w[3]);
    const int acc = (exp(-sw * beta[labels[r_begin + r]]) - u >= 0.0) ? 1 : 0;
    accept[r] = acc;
    work[4 * r + 2] += 1;
    if (!acc) work[4 * r + 3] += 1;
    work[4 * r + 1] = 0;
}
__global__ __launch_bounds__(256)
void metropolis_restore_kernel(int N, int Npad, const int* __restrict__ accept, float4* __restrict__ pos, float4* __restrict__ vel,
                               const float4* __restrict__ xold, const float4* __restrict__ vold)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (i >= N || accept[r]) return;
    const size_t o = (size_t)r * Npad + i;
    pos[o] = xold[o];
    const float4 v = vold[o];
    vel[o] = make_float4(-v.x, -v.y, -v.z, 0.f);
}
int remd_work_buffers(remd_ctx* h)
{
    if (h->d_work.size() == 4 * (size_t)h->R) return 0;
    REMD_TRY(h->d_work.alloc(h, 4 * (size_t)h->R));
    REMD_TRY(h->d_pe_prev.alloc(h, h->R));
    REMD_TRY(h->d_xold.alloc(h, (size_t)h->R * h->Npad));
    REMD_TRY(h->d_vold.alloc(h, (size_t)h->R * h->Npad));
    REMD_TRY(h->d_accept.alloc(h, h->R));
    REMD_CHECK(h, hipMemsetAsync(h->d_work, 0, sizeof(long long) * 4 * h->R, h->stream));
    return 0;
}

// Runs n_steps of the token program.  Tokens are grouped into chains that need no new
// force evaluation; a 'V' after an 'R' forces a force evaluation first.
//
// One loop body = one MD step's launches: the chain(s) around the centre-of-mass removal and the force evaluation on two streams.
// (Round 2 also captured the body into a hipGraph and replayed it: bit-identical and no faster on ROCm 7.2 -- the floor of a step is
// the dependent chain of kernels, not the host -- so the capture path was removed in round 3; DESIGN.md section 7b has the numbers.)
// The state remd_run_steps keeps between the MD steps of one call, as an object: begin() = everything in front of the step loop,
// step(s) = one MD step's launches, end() = the flush behind the last step.  One handle runs begin / step ... / end by itself
// (remd_run_steps); round 6: SEVERAL handles of one device take turns step by step from one host thread (remd_run_steps_many: the
// chain of one group of replicas beside the force kernels of another) -- nothing in here synchronises with the host.
struct step_runner {
    remd_ctx* h = nullptr; const unit_tables* ut = nullptr; const std::vector<char>* tokens = nullptr;
    int64_t first_step = 0; int n_steps = 0;
    chain_prog base{}, cur{};
    bool mts = false; unsigned group_mask[4] = {0u, 0u, 0u, 0u}; bool group_valid[4] = {false, false, false, false};
    bool shadow = false, pe_valid = false, zeroed_by_chain = false, device_waits_ok = false, merge_cmm = false;
    int cmm_w = 0; long long gstep0 = 0;
    bool done_by_resident = false;       // the resident small-system kernel took the whole call: step() / end() do nothing

    int begin(remd_ctx* h_, const std::vector<char>& tokens_, int nV, int nR, int nO, int64_t iteration, int64_t first_step_, int n_steps_)
    {
        h = h_; tokens = &tokens_; first_step = first_step_; n_steps = n_steps_;
        ut = &remd_table_of(h->units);
        if (ut->n_units == 0) return remd_fail(h, -3, "no system set");
        {
            const int rr = remd_run_steps_resident(h, tokens_, nV, nR, nO, iteration, first_step, n_steps);
            if (rr < 0) return rr;
            if (rr != 0) { done_by_resident = true; return 0; }
            const int rm = remd_run_steps_resident_mol(h, tokens_, nV, nR, nO, iteration, first_step, n_steps);
            if (rm < 0) return rm;
            if (rm != 0) { done_by_resident = true; return 0; }
        }
        base = chain_prog{};
        remd_step_prog_fill(base, {}, h->dt, h->gamma, nV, nR, nO);      // (no tokens: push() adds them chain by chain)
        base.cmm_r = -1; base.cmm_w = 0; base.zero_force = 0;
        // multiple-time-step program: one force array per force group that the splitting names, evaluated when a V of the group
        // comes up and the positions have changed since its last evaluation
        for (char c : tokens_) mts |= (c >= '0' && c <= '3');
        if (mts) {
            const size_t nf = (size_t)h->R * 3 * h->Npad;
            for (int g = 0; g < 4; ++g) {
                base.hVg[g] = h->nVg[g] > 0 ? (float)(h->dt / h->nVg[g]) : 0.f;
                for (int c = 0; c < 6; ++c) if (h->fgroup[c] == g) group_mask[g] |= 1u << c;
                if (h->n_restraints > 0 && h->rst_group == g) group_mask[g] |= 1u << REMD_FG_RESTRAINT;     // (restraints.hip)
                if (h->n_custom > 0 && h->cst_group == g) group_mask[g] |= 1u << REMD_FG_CUSTOM;            // (custom_terms.hip)
                if (h->nVg[g] > 0 && h->d_force_g[g].size() != nf) {
                    if (h->d_force_g[g]) REMD_CHECK(h, hipStreamSynchronize(h->stream));
                    REMD_TRY(h->d_force_g[g].alloc(h, nf));
                }
                base.Fg[g] = h->d_force_g[g];
            }
            unsigned named = 0u;
            for (int g = 0; g < 4; ++g) if (h->nVg[g] > 0) named |= group_mask[g];
            for (int c = 0; c < 6; ++c)
                if (h->fgroup[c] > 3 || !(named & (1u << c)))
                    return remd_fail(h, -3, "multiple-time-step splitting: a force class sits in a force group that no V of the splitting names "
                                            "(its forces would never act); groups 0-3 are supported");
            if (h->n_restraints > 0 && (h->rst_group > 3 || !(named & (1u << REMD_FG_RESTRAINT))))
                return remd_fail(h, -3, "multiple-time-step splitting: the restraints sit in a force group that no V of the splitting names "
                                        "(their forces would never act); groups 0-3 are supported");
            if (h->n_custom > 0 && (h->cst_group > 3 || !(named & (1u << REMD_FG_CUSTOM))))
                return remd_fail(h, -3, "multiple-time-step splitting: the custom forces sit in a force group that no V of the splitting names "
                                        "(their forces would never act); groups 0-3 are supported");
        }
        int n_braces = 0;
        for (char c : tokens_) n_braces += (c == '}');
        shadow = h->measure_shadow || n_braces > 0;                         // a Metropolized program measures shadow work (:1117-1119)
        base.measure = (h->measure_heat ? 1 : 0) | (shadow ? 2 : 0);
        if (base.measure) { int rcw = remd_work_buffers(h); if (rcw) return rcw; }
        pe_valid = false;                  // d_pe_prev holds U at the current positions
        cur = base; cur.n = 0;
        cmm_w = 0;                         // accumulator the next momentum sum goes to
        zeroed_by_chain = false;
        gstep0 = (long long)iteration * (long long)h->n_steps + first_step;
        // the centre-of-mass motion remover needs sum(m v) over the whole replica between two tokens of a step: either two launches
        // (the first ends with the sum) or one launch with a barrier over the replica's workgroups in device memory ('M' token) --
        // every workgroup of the grid must then be resident at once, hence the bound on the grid
        const long long chain_blocks = (long long)((ut->n_units + 255) / 256) * h->R;
        // (the same bound holds for the join polled in the chain's prologue: spinning workgroups of a grid larger than the chip
        // holds at once could keep the direct-space stream's last launches from ever being dispatched)
        device_waits_ok = chain_blocks <= 1024 && !h->no_device_waits;
        merge_cmm = h->sw.chain_merge && device_waits_ok && h->profiling != 2 && !h->lean_waits && !h->no_chain_barrier && !h->no_chain_merge;
        const long long sync_key = (long long)h->R * 1000003ll + ut->n_units;
        if (merge_cmm && (!h->d_chain_sync || h->chain_sync_key != sync_key)) {      // slots of THIS grid shape
            if (h->d_chain_sync) REMD_CHECK(h, hipStreamSynchronize(h->stream));
            h->chain_sync_key = sync_key;
            const size_t slots = 2 * (size_t)h->R * (size_t)((ut->n_units + 255) / 256) * 3;   // [2][R][workgroups][3]
            REMD_TRY(h->d_chain_sync.alloc(h, slots));
            REMD_CHECK(h, hipMemsetAsync(h->d_chain_sync, 0, sizeof(unsigned long long) * slots, h->stream));
            h->chain_sync_epoch = 0;
        }
        if (h->cmm_frequency > 0)
            hipMemsetAsync(h->d_cmm, 0, sizeof(long long) * 4 * 2 * h->R, h->stream);      // both accumulators, once per call
        return 0;
    }

    void flush(bool accumulate, bool bin_for_pme = false)      // bin_for_pme: a force evaluation follows this launch directly
    {
        if (cur.n == 0 && !accumulate) return;
        cur.accumulate_momentum = accumulate ? 1 : 0;
        cur.cmm_w = cmm_w;
        // forces are stale after an R that follows the chain's last V: let the chain clear them (saves a memset)
        bool seenR = false, staleAtEnd = false;
        for (int t = 0; t < cur.n; ++t) { if (cur.tok[t] == 'R') seenR = true; if (cur.tok[t] == 'V') seenR = false; }
        staleAtEnd = seenR && !mts;          // (the per-group arrays of a multiple-time-step program are cleared before their evaluation)
        cur.zero_force = staleAtEnd ? 1 : 0;
        if (staleAtEnd) zeroed_by_chain = true;
        launch_chain(h, *ut, cur, bin_for_pme);
        cur = base; cur.n = 0;
    }
    void push(char tok, int oidx, long long step)
    {
        if (cur.n == MAX_TOK) flush(false);
        cur.tok[cur.n] = tok; cur.o_index[cur.n] = oidx; cur.step[cur.n] = step; cur.n++;
    }
    int evaluate_with_energy(bool accumulate)
    {
        // energies (and forces) at the current positions; accumulate: add U - U_prev to the shadow work (:1420-1423)
        flush(false);
        h->force_zeroed = zeroed_by_chain;
        zeroed_by_chain = false;
        int rc = remd_compute_forces(h, true);
        if (rc) return rc;
        hipLaunchKernelGGL(work_pe_kernel, dim3((h->R + 63) / 64), dim3(64), 0, h->stream, h->R, h->d_potential, h->d_pe_prev, h->d_work, accumulate ? 1 : 0);
        pe_valid = true;
        return 0;
    }

    int step(int s)
    {
        if (done_by_resident) return 0;
        const long long gstep = gstep0 + s;
        // integrators.py:1313 addUpdateContextState: CMMotionRemover fires at the top of a step
        if (h->cmm_frequency > 0 && ((first_step + s) % h->cmm_frequency) == 0) {
            bool pending_reads_cmm = false;
            for (int t = 0; t < cur.n; ++t) pending_reads_cmm |= (cur.tok[t] == 'C');
            if (pending_reads_cmm) flush(false);   // it must see its own accumulator before the next sum starts
            if (merge_cmm && cur.n > 0 && cur.n + 2 <= MAX_TOK) {
                // ONE launch: pending tokens, 'M' (sum(m v) into buffer cmm_w + barrier over the replica's workgroups), 'C', ...
                push('M', 0, gstep);
                cur.m_buf = cmm_w; cur.m_epoch = ++h->chain_sync_epoch;
            } else {
                flush(true);                    // finishes pending tokens and accumulates sum(m v) into buffer cmm_w
            }
            push('C', 0, gstep);
            cur.cmm_r = cmm_w;                  // this chain subtracts P/M from that buffer and clears the other one
            cmm_w = 1 - cmm_w;
        }
        // Monte Carlo barostat (NPT states): acts in the same updateContextState slot, every baro_frequency-th step
        if (h->baro_frequency > 0 && (++h->baro_steps % h->baro_frequency) == 0) {
            flush(false);
            h->force_zeroed = zeroed_by_chain;
            zeroed_by_chain = false;
            int rc = remd_barostat_attempt(h);
            if (rc) return rc;
            for (bool& gv : group_valid) gv = false;
        }
        int oidx = 0, brace = 0;
        for (char tok : *tokens) {
            if (tok == '{') { push('{', 0, gstep); continue; }
            if (tok == '}') {
                flush(false);
                hipLaunchKernelGGL(metropolis_kernel, dim3((h->R + 63) / 64), dim3(64), 0, h->stream, h->R, h->r_begin, h->seed, gstep, brace++,
                                   h->d_labels, h->d_beta, h->d_work, h->d_accept, h->d_noise_id);
                hipLaunchKernelGGL(metropolis_restore_kernel, dim3((h->N + 255) / 256, h->R), dim3(256), 0, h->stream, h->N, h->Npad, h->d_accept,
                                   h->d_pos, h->d_vel, h->d_xold, h->d_vold);
                h->forces_valid = false; pe_valid = false;         // rejected replicas are back at their old positions
                for (bool& gv : group_valid) gv = false;
                continue;
            }
            if (tok == 'R' && shadow && !pe_valid) { int rc = evaluate_with_energy(false); if (rc) return rc; }
            if (tok >= '0' && tok <= '3' && !group_valid[tok - '0']) {
                // forces of this force group at the current positions, into the group's own array
                const int g = tok - '0';
                const bool has_mesh = (group_mask[g] >> REMD_FG_RECIPROCAL) & 1u;
                flush(false, has_mesh);
                std::swap(h->d_force, h->d_force_g[g]);      // (the evaluation fills the group's array)
                h->force_zeroed = false; zeroed_by_chain = false;
                int rc = remd_compute_forces(h, false, group_mask[g], device_waits_ok && !h->lean_waits);
                std::swap(h->d_force, h->d_force_g[g]);
                h->forces_valid = false; h->force_zeroed = false;      // (the all-forces accumulator was not touched)
                if (rc) return rc;
                group_valid[g] = true;
            }
            if (tok == 'V' && !h->forces_valid) {
                flush(false, true);
                h->force_zeroed = zeroed_by_chain;
                zeroed_by_chain = false;
                int rc = remd_compute_forces(h, false, ~0u, device_waits_ok && !h->lean_waits);   // (next on the main stream: the chain holding this V)
                if (rc) return rc;
            }
            push(tok, tok == 'O' ? oidx : 0, gstep);
            if (tok == 'O') oidx++;
            if (tok == 'R') {
                h->forces_valid = false;
                for (bool& gv : group_valid) gv = false;
                if (shadow) { int rc = evaluate_with_energy(true); if (rc) return rc; }
            }
        }
        return 0;
    }

    int end()
    {
        if (done_by_resident) return 0;
        flush(false);
        remd_launch_join_wait(h);
        { const int rc = remd_vsites_place(h, h->stream); if (rc) return rc; }     // (the positions this call leaves carry placed sites)
        h->force_zeroed = zeroed_by_chain;
        REMD_CHECK(h, hipGetLastError());
        return 0;
    }
};

// workgroups of one integrator-chain launch of this handle (one per 256 constraint units per replica)
long long remd_chain_blocks(remd_ctx* h)
{
    const unit_tables* ut = h->units.get();
    return ut ? (long long)((ut->n_units + 255) / 256) * h->R : 0;
}

int remd_run_steps(remd_ctx* h, const std::vector<char>& tokens, int nV, int nR, int nO,
                   int64_t iteration, int64_t first_step, int n_steps)
{
    step_runner sr;
    int rc = sr.begin(h, tokens, nV, nR, nO, iteration, first_step, n_steps);
    if (rc) return rc;
    for (int s = 0; s < n_steps && !sr.done_by_resident; ++s) {
        remd_nb_tune_step(h, n_steps - s);
        rc = sr.step(s); if (rc) return rc;
    }
    return sr.end();
}

// Several handles of ONE device, one host thread, the MD steps of the handles taking turns: handle 0's step s, handle 1's step s, ...
// Each handle keeps its own pair of streams, so the integrator chain of one group of replicas (a few hundred wavefronts waiting for one
// dependent thing after another) runs beside the pair and mesh kernels of another.  Nothing here waits for the device.
int remd_run_steps_many(remd_ctx** hs, int n, int64_t iteration, int64_t first_step, int n_steps)
{
    std::vector<step_runner> sr((size_t)n);
    for (int i = 0; i < n; ++i) {
        hipSetDevice(hs[i]->device);
        int rc = sr[i].begin(hs[i], hs[i]->tokens, hs[i]->nV, hs[i]->nR, hs[i]->nO, iteration, first_step, n_steps);
        if (rc) return rc;
    }
    for (int s = 0; s < n_steps; ++s)
        for (int i = 0; i < n; ++i) {
            if (sr[i].done_by_resident) continue;
            remd_nb_tune_step(hs[i], n_steps - s);
            int rc = sr[i].step(s); if (rc) return rc;
        }
    for (int i = 0; i < n; ++i) { int rc = sr[i].end(); if (rc) return rc; }
    return 0;
}

int remd_assign_velocities(remd_ctx* h, int64_t iteration)
{
    const unit_tables& ut = remd_table_of(h->units);
    remd_prof_scope ps(h, "assign_velocities");
    dim3 grid((ut.n_units + 255) / 256, h->R);
    hipLaunchKernelGGL(assign_velocities_kernel, grid, dim3(256), 0, h->stream, ut.n_units, ut.d_atoms, ut.d_type, ut.sc,
                       remd_constraint_tol(h), h->Npad, h->d_pos, h->d_vel, h->d_invmass, h->d_labels,
                       h->d_beta, h->r_begin, h->seed, iteration, h->d_noise_id);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

int remd_kinetic_energy(remd_ctx* h)
{
    remd_prof_scope ps(h, "kinetic_energy");
    hipLaunchKernelGGL(kinetic_energy_kernel, dim3(h->R), dim3(256), 0, h->stream, h->N, h->Npad, h->d_vel, h->d_mass, h->d_kinetic);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}

int remd_check_finite(remd_ctx* h)
{
    REMD_CHECK(h, hipMemsetAsync(h->d_nan, 0, sizeof(int) * h->R, h->stream));
    dim3 grid((h->N + 255) / 256, h->R);
    hipLaunchKernelGGL(check_finite_kernel, grid, dim3(256), 0, h->stream, h->N, h->Npad, h->d_pos, h->d_vel, h->d_nan);
    REMD_CHECK(h, hipGetLastError());
    return 0;
}
