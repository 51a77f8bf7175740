// Internal declarations of libremd_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <map>
#include <memory>
#include <vector>
#include "../../include/remd_hip.h"

#define REMD_KB 0.00831446261815324   // kJ/mol/K  (BOLTZMANN_CONSTANT_kB * AVOGADRO_CONSTANT_NA)
#define REMD_ONE_4PI_EPS0 138.93545764438198

struct remd_error { int code; std::string msg; };

struct remd_ctx;
void remd_set_global_error(const std::string& s);
int remd_hip_fail(remd_ctx* h, const char* what, hipError_t e);      // h->err and the global error, -2 (as REMD_CHECK)

// The one owner of a device allocation: move-only, freed by its destructor.  It converts to T* for kernel arguments, hipMemcpy*
// and pointer arithmetic; kernel argument structs hold the raw pointer, never this type.  alloc / upload / grow report a failed
// allocation through the handle and return -2.
template <typename T>
struct dev_array {
    dev_array() = default;
    dev_array(const dev_array&) = delete;
    dev_array& operator=(const dev_array&) = delete;
    dev_array(dev_array&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    dev_array& operator=(dev_array&& o) noexcept { if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(n_, o.n_); } return *this; }
    ~dev_array() { reset(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    void reset() { if (p_) hipFree(p_); p_ = nullptr; n_ = 0; }
    // exactly n elements, contents undefined (n = 0: none)
    int alloc(remd_ctx* h, size_t n)
    {
        reset();
        if (!n) return 0;
        const hipError_t e = hipMalloc(&p_, sizeof(T) * n);
        if (e != hipSuccess) { p_ = nullptr; return remd_hip_fail(h, "hipMalloc", e); }
        n_ = n;
        return 0;
    }
    // at least n elements; an array that is large enough is kept as it is
    int grow(remd_ctx* h, size_t n) { return n_ >= n && p_ ? 0 : alloc(h, n); }
    // a copy of `host` (empty: no allocation)
    int upload(remd_ctx* h, const std::vector<T>& host)
    {
        if (int rc = alloc(h, host.size())) return rc;
        if (host.empty()) return 0;
        const hipError_t e = hipMemcpy(p_, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice);
        return e == hipSuccess ? 0 : remd_hip_fail(h, "hipMemcpy", e);
    }
private:
    T* p_ = nullptr; size_t n_ = 0;
};

// what `expr` (an int status: 0 success) failed with, returned from the calling function
#define REMD_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)

// The feature tables a handle owns, each defined in the .hip file that builds it; the deleter of each is defined there too.
struct nb_tables; struct pme_state; struct unit_tables; struct gbsa_tables; struct nocutoff_tables; struct region_tables; struct rst_tables; struct cst_tables; struct vs_tables;
struct mix_pre_buffers;
struct remd_table_deleter {
    void operator()(nb_tables*) const; void operator()(pme_state*) const; void operator()(unit_tables*) const;
    void operator()(gbsa_tables*) const; void operator()(nocutoff_tables*) const; void operator()(region_tables*) const;
    void operator()(rst_tables*) const; void operator()(cst_tables*) const; void operator()(mix_pre_buffers*) const;
    void operator()(vs_tables*) const;
};
template <typename T> using remd_table = std::unique_ptr<T, remd_table_deleter>;
// a handle's table, made on first use
template <typename T> T& remd_table_of(remd_table<T>& t) { if (!t) t.reset(new T()); return *t; }

// fixed-point scale of the force accumulators (deterministic integer atomics)
#define REMD_FORCE_SCALE 4294967296.0   // 2^32
// what the X-H position solve is held to when the integrator asks for less: relative bond-length error of fp32 coordinates taken
// relative to the cluster's central atom (a few units in the last place of |r|^2)
#define REMD_CONSTRAINT_TOL_FLOOR 2e-7

// scaled fractional mesh coordinate u in [0, n) of a position component and its integer part: ONE definition, because the PME
// spreading pass recomputes the mesh column of an atom that was binned elsewhere (pme_bin_kernel or the integrator chain's
// epilogue) and the two must agree bit for bit
__device__ __forceinline__ void remd_pme_scaled1(float x, float L, int n, float& u, int& k)
{
    float f = x / L;
    f -= floorf(f);
    u = f * n;
    k = (int)u;
}
// what the integrator chain needs to bin the atoms it has just moved by mesh column kx (pme.hip owns the arrays):
// count[r][nx] (zero on entry) and atoms[r][nx][cap]; NULL count = no binning
// (an entry is the atom's position with its index in .w: the spreading pass then needs no second dependent load for it)
// (and its effective charge in a parallel array: no dependent load of the per-atom parameters either)
struct remd_chain_bins { int nx = 0, cap = 0; int* count = nullptr; float4* atoms = nullptr; const float* box = nullptr; unsigned int* err = nullptr;
                         float* q = nullptr; const float4* param = nullptr; const float* rep_lam = nullptr; };

// (unsigned long long)(long long)((double)f * 2^32), i.e. truncation toward zero, bit for bit, without the f64 conversion
// chain the cast expands to (8 double-rate instructions per component): |f| = floor + fraction is exact in f32, the
// fraction times 2^32 is exact, and the two halves are converted separately.  |f| >= 2^31 saturates as before.
__device__ __forceinline__ unsigned long long remd_f2fix(float f)
{
    const float a = fabsf(f);
    const float hi_f = floorf(a);
    const unsigned int lo = (unsigned int)((a - hi_f) * 4294967296.f);
    const unsigned int hi = (unsigned int)(int)hi_f;
    const unsigned long long v = ((unsigned long long)hi << 32) | lo;
    return f < 0.f ? 0ull - v : v;
}

// The join of the two streams without a launch of its own (round 4): the direct-space stream's last launch (the scatter of the
// pair kernel's sorted accumulators) has every workgroup count itself done with one atomic that nobody waits for, and the
// integrator chain's prologue polls that count instead of a flag published by a one-wavefront launch behind the scatter (5.6 us
// on what has become the critical path of a step).  Measured on the way and rejected: the scatter's LAST workgroup publishing the
// flag (it has to wait for its arrival atomic: 14 - 28 us), and the chain folding the sorted accumulators itself (no scatter
// launch at all, but +9 us in the one launch of a step that nothing overlaps): profiles/r04_h_rejected.txt, r04_p_fold_rejected.txt.
struct remd_fold_args {
    const unsigned int* done = nullptr; unsigned int target = 0;     // scatter workgroups finished (cumulative over launches)
};

struct listed_tables {
    int n_bonds, n_angles, n_torsions, n_exc, n_excl;
    const int *bond_atoms, *angle_atoms, *torsion_atoms, *exc_atoms, *excl_atoms;
    const float *bond_params, *angle_params, *torsion_params, *exc_params, *excl_qq;
    const int *exc_alch, *excl_alch; const float* rep_lam;
    float alpha, two_alpha_sqrtpi;
    // (term, slot) entries in the order of the atoms they act on (listed_terms.h); aterm NULL: one term per thread
    int n_aterm; const unsigned int* aterm;
};

// What remd_compute_forces (forces.hip) tells the mesh branch of an evaluation (remd_pme_forces, pme.hip).
struct remd_mesh_request {
    int part = 3;                      // 1: bin .. inverse z transform + gather, 2: the energy reduction, 3: both
    unsigned int fork_seq = 0;         // the fork flag that the first launch of part 1 publishes in d_sync[0] (0: none)
    listed_tables listed{}; int listed_total = 0;   // listed terms riding in the spreading launch as extra workgroups (0: none)
    bool prio_hi = true;               // the mesh kernels run at raised wave priority (false: the pair kernel does)
};

// What crosses from one launch function of an MD step to the next; everything else an evaluation decides is an argument.
struct remd_handover {
    // evaluation -> integrator chain: the join of a forked evaluation that the next main-stream launch still has to wait for, as the
    // join flag's sequence number (d_sync[1]) OR the scatter's done counter, never both.  launch_chain (integrate.hip) takes it as
    // a kernel argument, remd_launch_join_wait (forces.hip) turns what no chain took into a wait on the stream.
    struct wait_t { unsigned int seq = 0; remd_fold_args fold; } wait;
    bool cbins_ready = false;          // chain -> evaluation: the chain launched last binned the atoms for the PME pass that follows
    bool forked = false;               // the last evaluation ran on two streams (a fact, nothing pending: reset() keeps it)
    wait_t take_wait() { const wait_t w = wait; wait = wait_t(); return w; }
    bool take_bins() { const bool b = cbins_ready; cbins_ready = false; return b; }
    void reset() { wait = wait_t(); cbins_ready = false; }      // nothing is pending: positions or in-flight work were replaced
};

struct remd_profile_entry { int64_t n = 0; double ms = 0.0; };

// a deep copy of the descriptor of the last remd_set_system: the groups of replicas a handle propagates as phases (api.hip) are set up
// from it without the host
struct remd_desc_store {
    remd_system_desc d{}; bool valid = false;
    std::vector<double> mass, bond_params, angle_params, torsion_params, charge, sigma, epsilon, exception_params, shake_dist;
    std::vector<int32_t> ext_atoms, bond_atoms, angle_atoms, torsion_atoms, exception_atoms, settle_atoms, shake_atoms, alch_atoms;
    void assign(const remd_system_desc* s)
    {
        d = *s;
        auto cpd = [](std::vector<double>& v, const double*& p, size_t n) { if (p && n) { v.assign(p, p + n); p = v.data(); } else { v.clear(); if (!n) p = nullptr; } };
        auto cpi = [](std::vector<int32_t>& v, const int32_t*& p, size_t n) { if (p && n) { v.assign(p, p + n); p = v.data(); } else { v.clear(); if (!n) p = nullptr; } };
        const size_t N = (size_t)d.n_atoms;
        cpd(mass, d.mass, N); cpi(ext_atoms, d.ext_atoms, (size_t)d.n_ext);
        cpi(bond_atoms, d.bond_atoms, 2 * (size_t)d.n_bonds); cpd(bond_params, d.bond_params, 2 * (size_t)d.n_bonds);
        cpi(angle_atoms, d.angle_atoms, 3 * (size_t)d.n_angles); cpd(angle_params, d.angle_params, 2 * (size_t)d.n_angles);
        cpi(torsion_atoms, d.torsion_atoms, 4 * (size_t)d.n_torsions); cpd(torsion_params, d.torsion_params, 3 * (size_t)d.n_torsions);
        cpd(charge, d.charge, N); cpd(sigma, d.sigma, N); cpd(epsilon, d.epsilon, N);
        cpi(exception_atoms, d.exception_atoms, 2 * (size_t)d.n_exceptions); cpd(exception_params, d.exception_params, 3 * (size_t)d.n_exceptions);
        cpi(settle_atoms, d.settle_atoms, 3 * (size_t)d.n_settle);
        cpi(shake_atoms, d.shake_atoms, 4 * (size_t)d.n_shake); cpd(shake_dist, d.shake_dist, 3 * (size_t)d.n_shake);
        cpi(alch_atoms, d.alch_atoms, (size_t)d.n_alch);
        valid = true;
    }
};

// The environment switches the engine honours, read once per handle by remd_create (api.hip: read_switches) and copied
// to the blocks of a phased handle.  Test hooks that pin one of two bit-identical (or tolerance-equal) paths, the profiling tools'
// settings and diagnostic printers; nothing else under csrc/ reads the environment.  "Pinned" switches: n >= 0 pins the path
// (0 off, anything else on), unset or negative leaves the choice to the engine's rule.
struct remd_switches {
    bool overlap = true;          // REMD_OVERLAP=0: one stream, no fork of a PME force evaluation into a mesh and a direct-space stream
    int phases = -1;              // REMD_PHASES=n: overrides remd_set_phases (1 one block, 2 two, 0 by rule); unset: what remd_set_phases asked
    bool resident = true;         // REMD_RESIDENT=0: neither resident kernel (small systems, small molecules); the regular launches
    int resident_cap = 0;         // REMD_RESIDENT_CAP=n: the resident kernel's neighbour list holds at most n pairs (provokes its overflow path)
    bool chain_merge = true;      // REMD_CHAIN_MERGE=0: the centre-of-mass sum as two chain launches instead of a barrier inside one
    bool nb_tiles = false;        // REMD_NB_TILES set: the 64-atom tile pair kernel (a cluster-list overflow's fall-back) from the start
    int nb_persist_grid = -1;     // REMD_NB_PERSIST_GRID=n >= 0: the pair kernel's grid fixed (0: a workgroup per work item, else n resident
                                  //   workgroups pulling items) and the timing tuner off; unset: chosen by timing
    int nb_prio = -1;             // REMD_NB_PRIO, pinned: the pair kernel (1) or the mesh kernels (0) at raised wave priority; by default chosen by timing
    bool nb_fold = true;          // REMD_NB_FOLD=0: the integrator chain waits for a signal launch instead of polling the scatter's done counter
    bool listed_atoms = true;     // REMD_LISTED_ATOMS=0: listed terms one term per thread instead of (term, slot) entries in atom order
    bool listed_main = true;      // REMD_LISTED_MAIN=0: listed terms of a forked evaluation behind the pair kernel, not on the main stream
    bool listed_ride = true;      // REMD_LISTED_RIDE=0: listed terms as a launch of their own, not as workgroups of the spreading launch
    int pme_chainbin = -1;        // REMD_PME_CHAINBIN, pinned: mesh-column bins from the integrator chain's epilogue (0: the binning launch)
    int pme_cbin_cap = 0;         // REMD_PME_CBIN_CAP=n: at most n atoms per chain-binned mesh column (provokes the overflow path)
    int pme_pow2 = 3;             // REMD_PME_POW2 bits: 1 the register-resident plane pass, 2 the register-resident z passes of 64 / 128 meshes
    bool pme_fbin = true;         // REMD_PME_FBIN=0: mesh forces as scattered atomics per atom instead of by bin position
    bool gb_small = true;         // REMD_GB_SMALL=0: GBSA systems of up to 64 atoms take the three launches instead of one
    int mix_flow = -1;            // REMD_MIX_FLOW, pinned: the swap-all dataflow kernel (1) or the speculative windows (0); by default by acceptance
    bool mix_pre = true;          // REMD_MIX_PRE=0: speculative swap-all windows entirely in the serial workgroup (no hoisted mix_prep_kernel)
    bool debug = false;           // REMD_DEBUG set: print the cluster-pair list statistics after every re-sort
    bool nb_tune_verbose = false; // REMD_NB_TUNE_VERBOSE set: print the pair-kernel residency tuner's timings
    bool many_verbose = false;    // REMD_MANY_VERBOSE set: print host enqueue times of remd_propagate_many and the phases' stream set-up
    int prof_every = 16;          // REMD_PROF_EVERY=n: profiling level 1 samples every n-th launch of a class
};

struct remd_ctx {
    int device = 0;
    remd_switches sw;
    hipStream_t stream = nullptr; bool owns_stream = false;
    std::string err;
    uint64_t seed = 0;

    // ---- system -------------------------------------------------------------------
    int N = 0;            // atoms
    int Npad = 0;         // atoms padded to a multiple of 64
    bool has_system = false;
    dev_array<float> d_invmass;        // [Npad]  (0 for padding)
    dev_array<float> d_mass;           // [Npad]
    double total_mass = 0.0;
    // harmonic external force
    int n_ext = 0; dev_array<int> d_ext_atoms; double ext_K = 0, ext_x0 = 0, ext_U0 = 0;
    // bonded
    int n_bonds = 0, n_angles = 0, n_torsions = 0;
    dev_array<int> d_bond_atoms; dev_array<float> d_bond_params;
    dev_array<unsigned int> d_aterm; int n_aterm = 0;      // (term, slot) entries of the listed terms by atom (forces.hip: build_atom_terms)
    dev_array<int> d_angle_atoms; dev_array<float> d_angle_params;
    dev_array<int> d_torsion_atoms; dev_array<float> d_torsion_params;
    // nonbonded
    int nb_method = REMD_NB_NONE;
    int gbsa = 0;                      // remd_set_gbsa: GBSA (OBC2 + ACE) of a NoCutoff system (gbsa.hip)
    int nocutoff = 0;                  // the descriptor asked for REMD_NB_NOCUTOFF: nb_method stays REMD_NB_NONE for the rest of the engine, nocutoff.hip adds the direct sum
    double cutoff = 0, switch_dist = -1, rf_dielectric = 78.3, ewald_alpha = 0;
    int annihilate_sterics = 0;        // remd_set_alchemical_options: alchemical/alchemical sterics are lambda-controlled too
    int rf_unshifted = 0; double rf_switch_width = 0;   // remd_set_reaction_field: c_rf = 0, pair term switched over the last rf_switch_width nm
    double coulomb_cutoff = 0;         // remd_set_coulomb_cutoff: range of the Ewald direct-space sum (0: the NonbondedForce cutoff)
    int grid[3] = {0, 0, 0};
    int use_disp = 0;
    double disp_coeff = 0;             // E_lrc = disp_coeff / V for the non-alchemical system
    dev_array<float4> d_nbparam;       // [Npad] (q, sigma/2, 2*sqrt(eps), alch flag)
    dev_array<unsigned long long> d_exclmask; // [Npad][EXCL_WORDS] window exclusion bit masks
    int excl_window = 0;               // atoms j in [i-excl_window, i+excl_window] are mask-addressable
    int n_exceptions = 0;              // 1-4 style exceptions with non-zero params
    dev_array<int> d_exc_atoms; dev_array<float> d_exc_params;   // [n][2], [n][3]
    int n_excl_pairs = 0;              // all excluded pairs (for the PME exclusion correction)
    dev_array<int> d_excl_pairs;       // [n][2]
    double self_energy = 0;            // PME self term (kJ/mol), lambda_elec = 1
    // constraints
    int n_settle = 0; dev_array<int> d_settle_atoms; double settle_dOH = 0, settle_dHH = 0;
    int n_shake = 0;  dev_array<int> d_shake_atoms; dev_array<float> d_shake_dist;
    int n_groups = 0; dev_array<int> d_group_first;   // constraint groups (molecule-like units)
    dev_array<int> d_free_atoms; int n_free = 0;      // atoms in no constraint
    int cmm_frequency = 0;
    int n_dof = 0;
    // alchemy
    int n_alch = 0; dev_array<int> d_alch_atoms;
    double sc_alpha = 0.5, sc_a = 1, sc_b = 1, sc_c = 6;
    int n_regions = 0;                 // remd_set_alchemical_regions: general regions (alch_regions.hip holds the tables)
    int regions_exact = 0;             // ... under the exact PME treatment (the regions' scaled charges inside the Ewald sum)
    long long states_version = 0;      // bumped by every remd_set_states (restraints.hip: the restraint lambdas belong to one set of states)
    int n_restraints = 0, rst_group = 0;   // remd_set_restraints: receptor-ligand restraints and their force group (restraints.hip holds the tables)
    double cst_cutoff = 0;                 // the longest cutoff of a CutoffPeriodic CustomNonbondedForce (custom_nonbonded.hip): the box checks honour it
    int n_custom = 0, cst_group = 0;       // remd_set_custom_terms: custom bond / angle / torsion / external forces and their force group (custom_terms.hip)
    int n_massless = 0, n_vsites = 0;      // particles of mass 0 in the descriptor / sites declared by remd_set_virtual_sites (virtual_sites.hip): equal before anything runs

    // ---- states ---------------------------------------------------------------------
    int K = 0;
    std::vector<double> beta, lam_s, lam_e, econst;
    dev_array<double> d_beta; dev_array<double> d_lam_s; dev_array<double> d_lam_e; dev_array<double> d_econst;

    // ---- integrator -----------------------------------------------------------------
    std::string splitting = "V R O R V";
    std::vector<char> tokens;          // parsed 'V','R','O'
    int nV = 0, nR = 0, nO = 0;
    // multiple-time-step splittings (V0 V1 ..., integrators.py:1425-1442): tokens '0'..'3' = V of that force group;
    // nVg[g] = occurrences per step, fgroup[c] = force group of class c (REMD_FG_*), d_force_g[g] = that group's forces
    int nVg[4] = {0, 0, 0, 0};
    int fgroup[6] = {0, 0, 0, 0, 0, 0};
    dev_array<long long> d_force_g[4];
    double dt = 0.001, gamma = 1.0, constraint_tol = 1e-8;
    int n_steps = 1; int reassign = 1;
    bool has_integrator = false;
    // heat / shadow work / Metropolization (integrators.py:1175-1204, 1404-1460, 1539-1557)
    int measure_heat = 0, measure_shadow = 0;                   // (a splitting with '{' '}' measures shadow work whatever the flag says)
    dev_array<long long> d_snap_work;  // [2][R][4] remd_propagate: d_work at the start of the call / of each replica's successful attempt
    dev_array<long long> d_work;       // [R][4] fixed point 2^-24 kJ/mol: heat, shadow work; integers: Metropolis trials, rejections
    dev_array<double> d_pe_prev;       // [R] potential energy at the positions the last energy evaluation saw
    dev_array<float4> d_xold; dev_array<float4> d_vold; dev_array<int> d_accept;   // '{' snapshot, per-replica decision of '}'

    // ---- replicas -------------------------------------------------------------------
    int R_global = 0, r_begin = 0, R = 0;     // R = local replicas
    // remd_set_replica_ids: what keys the local replicas' random streams instead of r_begin + r (a handle that holds a
    // non-contiguous subset of an ensemble, multistate/_engine_pool.py); NULL: the block's own global indices
    dev_array<unsigned int> d_noise_id;
    dev_array<float4> d_pos;           // [R][Npad] xyz + pad
    dev_array<float4> d_vel;           // [R][Npad] xyz + pad
    // Monte Carlo barostat (OpenMM MonteCarloBarostat as the reference's NPT ThermodynamicState adds it, states.py:1177-1181)
    int baro_frequency = 0; long long baro_steps = 0, baro_attempts = 0; std::vector<double> pressure_host;   // (pressure_host: for the blocks of a phased propagation)
    double econst_vref = 0.0;          // volume at which the per-state energy constants were evaluated (they scale as 1/V); 0: constant
    dev_array<double> d_pressure;      // [K] kJ/mol/nm^3 (bar * N_A * 1e-25)
    dev_array<double> d_baro;          // [R][8]: volumeScale, attempted, accepted (adaptation window), total attempted, total accepted, dV, newV, oldV
    // per-axis barostats (include/remd_hip_barostat.h; barostat.hip): baro_kind 0 = the isotropic move above
    int baro_kind = 0, baro_axes = 0, baro_zmode = 0;     // (baro_axes: the anisotropic kind's scale mask / the membrane kind's xy mode)
    std::vector<double> tension_host;
    dev_array<double> d_tension;       // [K] kJ/mol/nm^2 (membrane kind)
    dev_array<double> d_baro_axis;     // [R][REMD_BARO_AXIS_STRIDE]: see barostat.hip
    dev_array<float> d_box_old; dev_array<float4> d_baro_x0; dev_array<long long> d_baro_f0; dev_array<double> d_baro_U0; dev_array<int> d_baro_acc;
    // rigid-body Monte Carlo moves (include/remd_hip_mcmoves.h; mc_moves.hip): the subsets of the last call, one after the other, and
    // the accepted flags [REMD_MC_MAX_MOVES][R]; the copies a rejection restores from are the barostat's (d_baro_x0, d_baro_f0, d_baro_U0)
    std::vector<int> mc_atoms_host; dev_array<int> d_mc_atoms; dev_array<int> d_mc_acc;
    bool box_uniform = false;          // every local replica has the same box (set_replicas; a barostat move clears it)
    int box_version = 0;               // bumped whenever the box edges on the device change (PME influence table)
    int n_restart_attempts = 0;        // mcmc.py:706-759
    dev_array<unsigned int> d_mix_log;      // swap-all attempt log (si, sj, accepted) when the counters do not fit
    bool mix_pre_launched = false, mix_no_pre = false;   // swap-all: the hoisted path ran last (its overflow flag is pending) / is off for the repeat
    double mix_acc_rate = -1.0;        // accepted / proposed of the previous swap-all call (picks the kernel of the next: mix.hip) in LDS
    dev_array<float4> d_snap_pos; dev_array<float4> d_snap_vel;   // pre-propagate state (restart attempts)
    dev_array<float4> d_fin_pos; dev_array<float4> d_fin_vel;     // first successful result of every replica
    dev_array<float> d_snap_box; dev_array<float> d_fin_box;      // boxes move under the barostat: same treatment
    dev_array<float4> d_pos_ref;       // [R][Npad] reference (constrained) positions for SHAKE/SETTLE
    dev_array<long long> d_force;      // [R][3][Npad] fixed point
    dev_array<float> d_box;            // [R][4] lx, ly, lz, pad
    std::vector<double> box_host;      // [R][3]
    dev_array<int64_t> d_labels;       // [R_global]
    std::vector<int64_t> labels;
    dev_array<double> d_ukl;           // [R_global][K]
    dev_array<double> d_potential;     // [R]
    dev_array<double> d_epart; int n_epart = 0;   // per-replica per-block energy partials
    dev_array<double> d_kinetic;       // [R]
    dev_array<int> d_nan;              // [R]
    dev_array<long long> d_cmm;        // [2][R][4] double-buffered fixed-point momentum accumulators
    bool forces_valid = false;
    bool force_zeroed = false;         // the last integrator chain already cleared d_force (skip the memset)

    // ---- feature tables, each defined in the file that owns it ------------------------------
    remd_table<pme_state> pme;         // pme.hip
    remd_table<nb_tables> nb;          // forces.hip: the nonbonded setup
    remd_table<unit_tables> units;     // constraint_units.h, built by integrate.hip: constraint units
    remd_table<nocutoff_tables> nc;    // nocutoff.hip
    remd_table<gbsa_tables> gb;        // gbsa.hip
    remd_table<region_tables> reg;     // alch_regions.hip
    remd_table<rst_tables> rst;        // restraints.hip
    remd_table<cst_tables> cst;        // custom_terms.hip
    remd_table<vs_tables> vs;          // virtual_sites.hip
    remd_table<mix_pre_buffers> mix_pre;   // mix.hip: the hoisted swap-all path

    // ---- mixing scratch ----------------------------------------------------------------
    dev_array<unsigned long long> d_nacc; dev_array<unsigned long long> d_nprop; int stats_K = 0;
    dev_array<double> d_logw; dev_array<double> d_logP; dev_array<double> d_ukl_tmp;

    // ---- timing / profiling -------------------------------------------------------------
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // second stream: the PME reciprocal pipeline (LDS / latency bound) overlaps the direct-space kernels (VALU bound)
    // fork / join of the two streams by flags in device memory ([0] fork, [1] join, [2] a spin ran out): the first mesh kernel
    // publishes the fork, a one-wavefront kernel at the head of the second stream waits for it, and the mirror image at the
    // join -- an event record / wait costs ~6 us of command-processor latency on the critical path, twice per step.
    // sync_events: the events instead, the fall-back of a handle whose polled wait ran out (api.hip: remd_recover_device_flag).
    dev_array<unsigned int> d_sync; unsigned int sync_seq = 0; bool sync_events = false;
    remd_handover next;
    // set when a wait polled on the device ran out / a capped PME bin overflowed: the handle falls back to events, two chain
    // launches and the binning launch (api.hip: remd_recover_device_flag) instead of staying dead behind a sticky flag
    bool no_device_waits = false, no_chain_bins = false, no_resident = false, no_chain_merge = false;
    // round 6, several handles propagated step by step from one host thread (remd_propagate_many): no workgroup of this handle may sit
    // on a CU polling for another stream while it holds registers another handle's kernels need -- the join is a one-wavefront launch
    // in front of the chain instead of a poll in the chain's prologue (320 registers per lane on every CU it occupies), the momentum
    // sum two launches instead of a barrier over resident workgroups
    bool lean_waits = false, no_chain_barrier = false;
    // ---- phases (round 6): remd_propagate of ONE handle as two groups of replicas whose MD steps take turns ------------------------
    // The local replicas are split into contiguous blocks, each block propagated by a child context of its own (full tables for its
    // share of the replicas; block 0 launches on THIS handle's two streams, block 1 on one more pair), the blocks' steps enqueued in
    // turn from the calling thread (remd_propagate_many): the integrator chain of one block runs beside the pair and mesh kernels
    // of the other.  Coordinates, velocities and the forces the last evaluation left go to the children device to device in front and
    // come back behind; everything else (energies, mixing, get / set) stays with this handle.  phases_req: remd_set_phases (0 = by rule).
    int phases_req = 0; int phases_last = 1;
    std::vector<remd_ctx*> phase; remd_ctx* parent = nullptr; int seen_parent_box = -1; long long ids_version = 0, seen_parent_ids = -1;     // (child: the parent's box_version its boxes were taken at)
    long long config_version = 0, phase_config = -1;      // children are rebuilt when a setter has run since they were made
    std::unique_ptr<remd_desc_store> sysdesc;
    std::vector<int64_t> noise_id_host;                   // remd_set_replica_ids, for the children's slices
    bool borrowed_stream2 = false;     // stream2 belongs to another handle (remd_adopt_streams): not destroyed with this one
    dev_array<unsigned long long> d_chain_own;   // [2] profiling: sum of (end - flag seen) wall-clock ticks of workgroup (0, 0), launches
    dev_array<unsigned long long> d_chain_sync; unsigned int chain_sync_epoch = 0; long long chain_sync_key = -1;    // [2][R][workgroups][3] epoch-tagged partial momentum sums of the 'M' token (integrate.hip)
    hipStream_t stream2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // sharding without a Python host (comm.hip): an RCCL communicator over the ranks of one replica-exchange run
    void* comm = nullptr; int comm_rank = 0, comm_world = 1;
    std::vector<long long> comm_begin, comm_count;   // every rank's block of replicas, exchanged when the local block changes
    dev_array<long long> d_comm_part; bool comm_part_current = false;
    double t_prop = 0, t_energy = 0, t_mix = 0;
    int profiling = 0;                 // 0 off, 1 filtered class only, 2 all classes
    std::string prof_filter = "nonbonded";
    std::map<const char*, long> prof_seen;
    struct pending_t { std::string name; hipEvent_t a, b; };
    std::vector<pending_t> prof_pending;
    std::map<std::string, remd_profile_entry> prof;

    remd_ctx() = default;
    remd_ctx(const remd_ctx&) = delete;
    remd_ctx& operator=(const remd_ctx&) = delete;
    ~remd_ctx();                       // api.hip: the phases, the communicator, pending profiling events, then the streams
};

#define REMD_CHECK(h, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
    (h)->err = std::string(#expr) + ": " + hipGetErrorString(_e); remd_set_global_error((h)->err); return -2; } } while (0)

void remd_set_global_error(const std::string& s);
int remd_fail(remd_ctx* h, int code, const std::string& msg);
// the tolerance every constraint solve of this handle is launched with
inline float remd_constraint_tol(const remd_ctx* h) { return (float)fmax(h->constraint_tol, REMD_CONSTRAINT_TOL_FLOOR); }
void remd_comm_release(remd_ctx* h);      // comm.hip

// profiling wrapper: brackets a launch with HIP events recorded on the handle's stream.  Nothing is
// synchronised at launch time; the pairs are resolved in remd_profile_get().  Level 1 records only
// the class named by prof_filter (bench.py: the dominant kernel), level 2 records every class.
struct remd_prof_scope {
    remd_ctx* h; const char* name; hipEvent_t a = nullptr; bool on = false; hipStream_t st;
    remd_prof_scope(remd_ctx* h_, const char* n, hipStream_t stream = (hipStream_t)-1) : h(h_), name(n) {
        st = (stream == (hipStream_t)-1) ? h->stream : stream;     // events go on the stream the kernel is launched on
        on = h->profiling == 2;
        if (h->profiling == 1) {                       // filter: '|'-separated class-name prefixes
            const std::string nm(n), &f = h->prof_filter;
            for (size_t b = 0; b <= f.size() && !on; ) {
                size_t e = f.find('|', b); if (e == std::string::npos) e = f.size();
                on = e > b && nm.compare(0, e - b, f, b, e - b) == 0;
                b = e + 1;
            }
            // sampled: every sw.prof_every-th launch of a class (an event pair costs host time and, on the main stream, ~12 us of
            // command-processor latency on the critical path of a step: timing every launch slows what it measures)
            if (on) on = (h->prof_seen[n]++ % h->sw.prof_every) == 0;
        }
        if (on) { hipEventCreate(&a); hipEventRecord(a, st); }
    }
    ~remd_prof_scope() {
        if (on) {
            hipEvent_t b; hipEventCreate(&b); hipEventRecord(b, st);
            h->prof_pending.push_back({name, a, b});
        }
    }
};

// ---- mix.hip --------------------------------------------------------------------------
int remd_mix_launch(remd_ctx* h, int scheme, int64_t iteration, int R, int K, int ld, const double* d_ukl,
                    int64_t* d_labels, unsigned long long* d_nacc, unsigned long long* d_nprop,
                    const double* d_logw, double* d_logP, int64_t n_attempts);
const unsigned* remd_mix_pending_flag(remd_ctx* h);

// ---- integrate.hip ----------------------------------------------------------------------
int remd_parse_splitting(remd_ctx* h, const char* splitting, std::vector<char>& tokens, int& nV, int& nR, int& nO, int* nVg = nullptr);
int remd_run_steps(remd_ctx* h, const std::vector<char>& tokens, int nV, int nR, int nO,
                   int64_t iteration, int64_t first_step, int n_steps);
int remd_run_steps_many(remd_ctx** hs, int n, int64_t iteration, int64_t first_step, int n_steps);   // the handles' steps taking turns
long long remd_chain_blocks(remd_ctx* h);            // workgroups of one integrator-chain launch
int remd_assign_velocities(remd_ctx* h, int64_t iteration);
int remd_kinetic_energy(remd_ctx* h);
int remd_check_finite(remd_ctx* h);
int remd_work_buffers(remd_ctx* h);                    // heat / shadow-work accumulators and the '{' snapshot of the local replicas
int remd_build_constraints(remd_ctx* h, const remd_system_desc* d);
int remd_check_settle_masses(remd_ctx* h, const remd_system_desc* d);      // 0, or remd_fail(-3): nothing of the handle changed

// ---- resident.hip: a whole propagation in one launch ------------------------------------------
// each returns 1 when it ran the propagation, 0 when the system / request is not one it covers, < 0 on error
int remd_run_steps_resident(remd_ctx* h, const std::vector<char>& tokens, int nV, int nR, int nO,
                            int64_t iteration, int64_t first_step, int n_steps);
int remd_run_steps_resident_mol(remd_ctx* h, const std::vector<char>& tokens, int nV, int nR, int nO,
                                int64_t iteration, int64_t first_step, int n_steps);

// ---- minimize.hip -----------------------------------------------------------------------
int remd_minimize_impl(remd_ctx* h, double tolerance, int max_iterations, int32_t* converged, int32_t* n_iterations);

// ---- forces.hip -------------------------------------------------------------------------
int remd_barostat_attempt(remd_ctx* h);                      // barostat.hip
int remd_barostat_buffers(remd_ctx* h);                      // (its per-replica state and scratch, allocated on first use)
#define REMD_BARO_AXIS_STRIDE 24
struct remd_mc_move_desc;
int remd_mc_moves_enqueue(remd_ctx* h, const remd_mc_move_desc* moves, int n_moves, int64_t iteration);   // mc_moves.hip: checked, then enqueued; flags in d_mc_acc
int remd_tension_ukl(remd_ctx* h, double* d_rows);           // membrane barostat: - beta_l gamma_l A_xy(r) into the u_kl rows
int remd_nb_molecules(remd_ctx* h, const int** first, const int** size);   // molecule table of the nonbonded setup (device); 0: none
void remd_nb_invalidate_sort(remd_ctx* h);            // the next force evaluation re-sorts the molecules
void remd_nb_reset_accumulators(remd_ctx* h);         // after a device-side fault: the sorted accumulators of a discarded evaluation
void remd_nb_tune_step(remd_ctx* h, int steps_left_in_call);   // the pair kernel's residency, chosen by timing
void remd_nb_tune_resolve(remd_ctx* h);
struct nb_params;                                     // pair_math.h
int remd_nb_resident_info(remd_ctx* h, int* ok, int* method, int* has_alch, nb_params* p, const float4** param, const float** rep_lam);
const float* remd_nb_rep_lam(remd_ctx* h);            // what the mesh kernels read: per-replica lambdas (NULL: none) ...
const float4* remd_nb_param(remd_ctx* h);             // ... and per-atom parameters
int remd_nb_required_epart(remd_ctx* h);
int remd_assemble_ukl(remd_ctx* h, double* d_rows);
void remd_launch_join_wait(remd_ctx* h);              // a join left for an integrator chain that no chain took (remd_handover::wait)
// force classes (bits of the mask of remd_compute_forces, indices of remd_ctx::fgroup)
#define REMD_FG_EXTERNAL 0
#define REMD_FG_BOND 1
#define REMD_FG_ANGLE 2
#define REMD_FG_TORSION 3
#define REMD_FG_NONBONDED 4      /* direct space, exceptions, Ewald exclusion correction */
#define REMD_FG_RECIPROCAL 5
#define REMD_FG_RESTRAINT 6      /* receptor-ligand restraints (restraints.hip), force group remd_ctx::rst_group */
#define REMD_FG_CUSTOM 7         /* custom bond / angle / torsion / external forces (custom_terms.hip), force group remd_ctx::cst_group */
// nocutoff.hip: NonbondedForce with NoCutoff (vacuum systems)
int remd_nocutoff_build(remd_ctx* h, const remd_system_desc* d);
int remd_nocutoff_forces(remd_ctx* h, bool with_energy, int ep_slot);
int remd_nocutoff_info(remd_ctx* h, const float4** param, const unsigned int** excl, int* words, int* n_exc, const int** exc_atoms, const float4** exc_par);
// gbsa.hip: implicit solvent of a NoCutoff system
int remd_gbsa_forces(remd_ctx* h, bool with_energy, int ep_slot);
int remd_gbsa_ukl(remd_ctx* h, double* d_alch /*[R][K], added to*/);
int remd_regions_state_le(remd_ctx* h, int k, int g, double* le);
// alch_regions.hip: custom forces of general alchemical regions
void remd_regions_release(remd_ctx* h);                // drops the regions (remd_set_system)
int remd_regions_clone(remd_ctx* parent, remd_ctx* child);
int remd_gbsa_clone(remd_ctx* parent, remd_ctx* child);
int remd_regions_forces(remd_ctx* h, bool with_energy, int ep_slot);
int remd_regions_ukl(remd_ctx* h, double* d_out /*[R][K]*/, const int** d_own);
int remd_regions_pme_tables(remd_ctx* h, const float4** param, const float** rep_le);
int remd_regions_le_override(remd_ctx* h, const float* le, int* n, const float** d_state_le);
// fills d_force (and d_potential when with_energy).  chain_follows: the caller's next launch on the main stream is an integrator
// chain of this handle, so the join of a forked evaluation may be left in h->next.wait for that chain to poll
int remd_compute_forces(remd_ctx* h, bool with_energy, unsigned class_mask = ~0u, bool chain_follows = false);
int remd_build_nonbonded(remd_ctx* h, const remd_system_desc* d);

// restraints.hip: receptor-ligand restraints (include/remd_hip_restraints.h); their energy partial is the LAST slot of d_epart
void remd_restraints_release(remd_ctx* h);
int remd_restraints_clone(remd_ctx* parent, remd_ctx* child);
int remd_restraints_forces(remd_ctx* h, bool with_energy, int ep_slot, hipStream_t st);
int remd_restraints_ukl(remd_ctx* h, double* d_rows /*[R][K], added to*/);

// custom_terms.hip: custom bond / angle / torsion / external forces (include/remd_hip_custom.h); their energy joins the restraints'
// slot of d_epart, added behind the restraint launch on the same stream
void remd_custom_release(remd_ctx* h);
int remd_custom_clone(remd_ctx* parent, remd_ctx* child);
int remd_custom_molecules(remd_ctx* h, const int** first, const int** size);   // molecule table of a handle whose only pair force is a periodic CustomNonbondedForce (device); 0: none
int remd_custom_forces(remd_ctx* h, bool with_energy, int ep_slot, hipStream_t st);
int remd_custom_ukl(remd_ctx* h, double* d_rows /*[R][K], added to*/);

// virtual_sites.hip: virtual sites (include/remd_hip_vsites.h); both launches are skipped by a handle without sites
void remd_vsites_release(remd_ctx* h);
int remd_vsites_clone(remd_ctx* parent, remd_ctx* child);
int remd_vsites_place(remd_ctx* h, hipStream_t st, bool zero_velocities = false);   // every site from its parents' current positions
int remd_vsites_spread(remd_ctx* h, hipStream_t st);      // the sites' words of d_force to their parents, zero left behind

// ---- pme.hip ----------------------------------------------------------------------------
int remd_pme_setup(remd_ctx* h);
int remd_pme_forces(remd_ctx* h, bool with_energy, hipStream_t st, const remd_mesh_request& rq);
remd_chain_bins remd_pme_chain_bins(remd_ctx* h);     // bins for the next evaluation, to be filled by the integrator chain in front of it
int remd_test_fft3d_impl(remd_ctx* h, int nx, int ny, int nz, float* data, int inverse);
