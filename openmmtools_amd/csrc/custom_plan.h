// The host set-up of the custom forces (include/remd_hip_custom.h): what remd_set_custom_terms checks and lays out before anything
// touches the device.  Plain C++17 with no HIP header, so tools/custom_plan_check.cpp runs it under the host compiler's sanitizers
// (tests/test_custom_plan_cpu.py).  cst_build_plan maps the descriptors, and the few facts of the handle it needs, to a filled
// cst_plan or to the sentence of the refusal; custom_terms.hip uploads the plan's tables as they stand (cst_tables, custom_machine.h).
// The kernels index the stack, the constants, the parameters, the atoms, the groups, the maps and the exclusion rows unchecked: what
// a descriptor may name is settled here, once.
//
// A new kind: its REMD_CUSTOM_* value gets an entry in cst_part_of_kind, cst_width and cst_n_vars (and a cst_part of its own where it
// has a kernel of its own), a validator beside cst_check_cmap called from cst_check_force, its share of cst_pack_force, and its
// tables as members of cst_plan with one line in upload_tables (custom_terms.hip).  Nothing else lists the tables.  The donor-acceptor kind
// (REMD_CUSTOM_HBOND) keeps its validator, its share of the packing and its molecules in custom_hbond_plan.h, included below, and the
// many-particle kind (REMD_CUSTOM_MANYPARTICLE) its validator and packer in custom_manyparticle_plan.h, the Generalized-Born kind
// (REMD_CUSTOM_GB) its own in custom_gb_plan.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../../include/remd_hip_custom.h"

struct cst_force {
    int kind, periodic, n_terms, n_params;
    int n_particles;             // atoms per term (the particles per bond of a compound-bond force, the groups per bond of a centroid force)
    int slot0, npad;             // first slot in the padded term space of the launch / slots of this force (a multiple of 64)
    int par0;                    // offset of its parameters [n_params][npad]
    int prog0, n_prog, const0;   // its program and constants in the handle's tables
    // REMD_CUSTOM_NONBONDED only (custom_nonbonded.hip): n_terms = N particles, npad = 64 x its upper-triangular tiles, parameters [n_params][Npad]
    int nb_method;               // 0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic
    int excl0;                   // its row offsets [N + 1] in the handle's excl_off (which point into the handle's excl_atoms)
    int lrc;                     // 1: it has a long-range correction (the handle's lrc table carries its column)
    double cutoff, switch_dist;  // switch_dist < 0: no switching function
    // REMD_CUSTOM_CV only (custom_cv.hip): n_terms = 1, npad = 64, no atoms of its own
    int cv0, n_cvs;              // its first collective variable among the handle's, and how many it has (1 ... 3)
    // REMD_CUSTOM_CMAP only (cmap.hip): n_particles = 8, no program and no parameters; its constants are its maps' blocks
    int map0, n_maps;            // its first map among the handle's map_off, and how many it has (1 ... REMD_CUSTOM_MAX_MAPS)
    // REMD_CUSTOM_HBOND only (custom_hbond.hip): n_terms = donors, npad = 64 x its tiles (donor blocks x acceptor blocks, row by row);
    // it shares nb_method, cutoff and excl0 (its rows [donors + 1] in excl_off, acceptor indices in excl_atoms) with the nonbonded kind
    int hb_na;                   // acceptors
    int hb_atoms0;               // in the handle's hb_atoms: donors [3][ndpad], then acceptors [3][napad] (ndpad = 64 ceil(donors / 64), ...)
    int hb_npd, hb_npa;          // per-donor and per-acceptor parameters: [hb_npd][ndpad] at par0, then [hb_npa][napad]
    int hb_mask;                 // bit s: the program names particle slot s (d1 d2 d3 a1 a2 a3 = 0 ... 5); one seeded pass per bit
    // REMD_CUSTOM_MANYPARTICLE only (custom_manyparticle.hip): n_terms = N particles, npad = 64 N (one wavefront per central particle),
    // parameters [n_params][Npad]; it shares nb_method, cutoff and excl0 (rows [N + 1], symmetric, sorted) with the nonbonded kind
    int mp_mode;                 // 0 SinglePermutation, 1 UniqueCentralParticle
    int mp_types0;               // its types [Npad] in the handle's mp_types
    int mp_row0;                 // its first neighbour row among the handle's (Npad rows per such force)
    int mp_mask;                 // bit s: the program names particle slot s (p1 p2 p3 = 0 1 2); one seeded pass per bit
    unsigned mp_filter[3];       // per slot: bit t set where type t may fill it
    // REMD_CUSTOM_GB only (custom_gb.hip): n_terms = N particles, npad = 64 nb (gb_slices + 1), parameters [n_params][Npad]; it shares
    // nb_method, cutoff and excl0 (rows [N + 1], symmetric, sorted) with the nonbonded kind
    int gb_n_values, gb_n_stages;  // its computed values and the rows of its stage table
    int gb_stage0;               // its first row in the handle's gb_stages
    int gb_slices;               // column slices of its pair launches (cst_gb_slices)
    long long gb_work0;          // its first double in a replica's share of the handle's gb work buffer
};

// The parts of the padded term space, in its order; each has its own kernels, which run the wavefronts [begin(part), end(part)).
enum cst_part { CST_SIMPLE, CST_COMPOUND, CST_NONBONDED, CST_CENTROID, CST_CV, CST_CMAP, CST_HBOND, CST_MANYPARTICLE, CST_GB, CST_N_PARTS };
// indexed by REMD_CUSTOM_*: the part of a kind (the four one-variable kinds share the first)
// (kind 9 is not assigned and never gets this far: cst_check_shape refuses it; its entries below only keep the tables indexed by kind)
static const int cst_part_of_kind[REMD_CUSTOM_GB + 1] = {CST_SIMPLE, CST_SIMPLE, CST_SIMPLE, CST_SIMPLE, CST_COMPOUND, CST_CENTROID, CST_NONBONDED, CST_CV, CST_CMAP, CST_HBOND, CST_HBOND, CST_MANYPARTICLE, CST_GB};

// everything the set-up computes on the host; the energy columns keep the forces' order whatever their slots
struct cst_plan {
    int nf = 0, ng = 0, K = 0, total_pad = 0; long long glob_version = -1;   // (glob belongs to the states of that remd_set_states)
    int part_end[CST_N_PARTS] = {};    // in wavefronts: where each part of the padded term space ends (the next one begins there)
    int begin(int part) const { return part ? part_end[part - 1] : 0; }
    int end(int part) const { return part_end[part]; }
    bool has(int part) const { return end(part) > begin(part); }
    int n_cv = 0;                      // the collective variables of all such forces (0: no such force, none of the cv members below holds anything)
    int n_groups = 0;                  // the groups of all centroid forces (0: no centroid force, none of the grp / ref members below holds anything)
    bool uniform = true;               // every state carries the same globals: no u_kl share
    // energy parameter derivatives (remd_set_custom_parameter_derivatives): the distinct global columns asked for, and per force the
    // mask of those it declared (bit d: column dcols[d]); a force contributes to a derivative only where its bit is set.  Empty: none.
    std::vector<int> dcols; std::vector<unsigned> dmask;
    std::vector<cst_force> F; std::vector<int> wave_force;
    std::vector<int> atoms;            // [max(4, most particles per bond)][total_pad]; a padding slot repeats the force's last term
    std::vector<double> par, consts, glob, defaults;
    std::vector<int> prog;             // (opcode, operand) pairs: the kernels' int2
    // centroid forces (custom_centroid.hip): a centroid force's row of `atoms` holds handle-wide group numbers
    std::vector<int> grp_off;          // [n_groups + 1] into grp_atoms / grp_w
    std::vector<int> grp_atoms; std::vector<double> grp_w;      // the groups' atoms and their weights (sum 1 per group)
    std::vector<int> grp_periodic;     // [n_groups]: the flag of the force the group belongs to
    std::vector<int> ref_off;          // [n_groups + 1] into refs
    std::vector<int> refs;             // (centroid slot * REMD_CUSTOM_MAX_PARTICLES + position in the bond) of every bond that names the group, in table order
    // collective-variable forces (custom_cv.hip): the RMSD variables of all of them in CSR form (cst_force::cv0 names a force's first)
    std::vector<int> cv_off;           // [n_cv + 1] into cv_atoms / cv_ref
    std::vector<int> cv_atoms;         // the variables' particles
    std::vector<double> cv_ref;        // beside cv_atoms, [.][3]: the reference, centred on each variable's own centroid
    // CMAP forces (cmap.hip): the maps of all of them and the map of every slot of their part of the padded term space
    std::vector<int> map_off;          // per map the offset of its block in consts (cst_force::map0 names a force's first)
    std::vector<int> map_index;        // [64 (end(CST_CMAP) - begin(CST_CMAP))]: the slot's map among its force's, 0 ... n_maps - 1 (a padding slot repeats the last term's)
    // nonbonded forces (custom_nonbonded.hip): the exclusion rows of all of them, and the long-range coefficients of the states
    std::vector<int> excl_off;         // per nonbonded force N + 1 offsets into excl_atoms (cst_force::excl0 names the first)
    std::vector<int> excl_atoms;       // symmetric, sorted within a row
    std::vector<double> lrc;           // [K][nf] kJ/mol nm^3: the energy is lrc[state][force] / V (zero for a force without the correction)
    // donor-acceptor forces (custom_hbond.hip): per force the donors' particles [3][ndpad], then the acceptors' [3][napad]; -1: the donor
    // (acceptor) has no such particle; a padding column repeats the last donor (acceptor).  Their exclusion rows join excl_off / excl_atoms.
    std::vector<int> hb_atoms;
    // many-particle forces (custom_manyparticle.hip): per force the particles' types [Npad] (a padding column repeats the last atom's),
    // and the neighbour rows of all of them (Npad per force; the rows themselves are work buffers on the device).  Their exclusion
    // rows join excl_off / excl_atoms.
    std::vector<int> mp_types;
    int mp_rows = 0;
    // Generalized-Born forces (custom_gb.hip): the stage rows of all of them, and the doubles of work buffer one replica needs for
    // all of them (custom_gb_plan.h).  Their exclusion rows join excl_off / excl_atoms.
    std::vector<int> gb_stages;
    size_t gb_work = 0;
    bool has_lrc = false, lrc_valid = false;   // (lrc_valid: remd_set_custom_lrc ran since the globals were last set)
    double periodic_cutoff = 0.0;      // the longest cutoff of a CutoffPeriodic nonbonded, donor-acceptor or many-particle force (remd_ctx::cst_cutoff)
    // the molecules a barostat moves as wholes where the handle has no NonbondedForce to take them from (remd_custom_molecules): atoms
    // the custom bonds, angles, torsions and compound bonds join, each a contiguous range [first, first + size); empty: no table
    std::vector<int> mol_first, mol_size;
};

// what the set-up needs to know of the handle
struct cst_facts {
    int N, Npad, K; long long states_version;
    const double* boxes; size_t n_boxes;   // the host's copy of the box edges, all replicas' (n_boxes = 0: none yet)
    bool bare;                             // no built-in nonbonded force, listed terms or constraints: the custom bonds alone make the molecules
};

inline bool cst_is_compound(int kind) { return kind == REMD_CUSTOM_COMPOUND || kind == REMD_CUSTOM_CENTROID; }
// atoms (group numbers) per term in the descriptor's `atoms`
inline int cst_width(const remd_custom_force_desc& d)
{
    static const int width[REMD_CUSTOM_GB + 1] = {2, 3, 4, 1, -1, -1, 0, 0, 8, 0, 0, 0, 0};
    return cst_is_compound(d.kind) ? d.n_particles : width[d.kind];
}
// the variables a program may name
inline int cst_n_vars(const remd_custom_force_desc& d)
{
    static const int n_vars[REMD_CUSTOM_GB + 1] = {1, 1, 1, 3, -1, -1, 1, -1, 0, 0, 0, 0, 3};
    return cst_is_compound(d.kind) ? 3 * d.n_particles : d.kind == REMD_CUSTOM_CV ? d.n_cvs : n_vars[d.kind];
}

#include "custom_hbond_plan.h"     // the donor-acceptor kind's validator, packer and molecules (cst_check_hbond, cst_pack_hbond, cst_hbond_molecules)
#include "custom_manyparticle_plan.h"   // the many-particle kind's validator and packer (cst_check_manyparticle, cst_pack_manyparticle)

// the block of the function at consts[arg] (include/remd_hip_custom.h): the kernels trust n, min, max and the block's extent
inline const char* cst_check_table1d(const remd_custom_force_desc& d, int op, int arg)
{
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
    return nullptr;
}

// the same for the blocks of two and three arguments: the sizes, their product, the bounds and the extent
inline const char* cst_check_table2d3d(const remd_custom_force_desc& d, int op, int arg)
{
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
    return nullptr;
}

// what a program may do is settled here, once: the kernels index the stack, the constants, the parameters and the globals unchecked
inline const char* check_program(const remd_custom_force_desc& d, int n_vars)
{
    const int n_par = d.kind == REMD_CUSTOM_NONBONDED ? 2 * d.n_params                   // (a pair: particle 1's parameters, then particle 2's)
                    : d.kind == REMD_CUSTOM_HBOND ? d.hb_n_donor_params + d.hb_n_acceptor_params                 // (the donor's, then the acceptor's)
                    : d.kind == REMD_CUSTOM_MANYPARTICLE ? 3 * d.n_params : d.n_params;                           // (operand 3 q + s: parameter q of slot s)
    if (d.n_program <= 0 || !d.program) return "an empty program";
    if (d.n_program > REMD_CUSTOM_MAX_PROGRAM) return "a program over REMD_CUSTOM_MAX_PROGRAM instructions";
    int sp = 0, top = 0;
    for (int pc = 0; pc < d.n_program; ++pc) {
        const int op = d.program[2 * pc], arg = d.program[2 * pc + 1];
        const char* bad = nullptr;
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
            const bool hbond = d.kind == REMD_CUSTOM_HBOND, many = d.kind == REMD_CUSTOM_MANYPARTICLE;
            if (!cst_is_compound(d.kind) && !hbond && !many) return "a function of particles outside a compound-bond or centroid-bond force";
            const int n_args = op - REMD_CX_DISTANCE + 2;
            if (arg < 0 || (arg >> (4 * n_args)) != 0) return "a particle slot out of range";
            for (int k = 0; k < n_args; ++k) {
                const int slot = (arg >> (4 * k)) & 15;
                if (slot >= (hbond ? 6 : many ? 3 : d.n_particles)) return "a particle slot out of range";
            }
            pops = 0;
        } break;
        case REMD_CX_POWI: if (arg < -64 || arg > 64) return "an integer power beyond +-64"; break;
        case REMD_CX_TABLE1D: case REMD_CX_LOOKUP1D: bad = cst_check_table1d(d, op, arg); break;
        case REMD_CX_TABLE2D: case REMD_CX_LOOKUP2D: case REMD_CX_LOOKUP3D: bad = cst_check_table2d3d(d, op, arg); pops = op == REMD_CX_LOOKUP3D ? 3 : 2; break;
        default: if (op < 0 || op >= REMD_CX_N_OPCODES) return "an unknown opcode"; break;
        }
        if (bad) return bad;
        if (sp < pops) return "a program that pops an empty stack";
        sp += 1 - pops;
        top = std::max(top, sp);
        if (sp > REMD_CUSTOM_MAX_STACK) return "a program over REMD_CUSTOM_MAX_STACK stack slots";
    }
    if (sp != 1) return "a program that does not leave exactly one value";
    if (top != d.stack_depth) return "a stack depth that is not the program's";
    return nullptr;
}

#include "custom_gb_plan.h"            // the Generalized-Born kind's validator and packer (cst_check_gb, cst_pack_gb); it runs check_program per stage

// The validators: each returns the sentence of the first fault, or nothing.  cst_check_force fixes their order.

// every kind: the kind itself, the particles per term, the terms, the per-term parameters
inline std::string cst_check_shape(const remd_custom_force_desc& d)
{
    if (d.kind < 0 || d.kind > REMD_CUSTOM_GB || d.kind == REMD_CUSTOM_CMAP + 1) return "unknown kind";      // (9 is not assigned)
    const bool cmap = d.kind == REMD_CUSTOM_CMAP, atomless = d.kind == REMD_CUSTOM_NONBONDED || d.kind == REMD_CUSTOM_CV || d.kind == REMD_CUSTOM_HBOND || d.kind == REMD_CUSTOM_MANYPARTICLE || d.kind == REMD_CUSTOM_GB;
    if (cmap && d.n_particles != 8) return "n_particles is 8 for a CMAP force (two dihedrals of four particles)";
    if (!cmap && (cst_is_compound(d.kind) ? (d.n_particles < 1 || d.n_particles > REMD_CUSTOM_MAX_PARTICLES) : d.n_particles != 0))
        return "n_particles is 1 ... REMD_CUSTOM_MAX_PARTICLES for a compound-bond or centroid-bond force and 0 for every other kind";
    if (d.n_terms <= 0 || (!d.atoms && !atomless)) return "no terms";
    if (d.n_params < 0 || d.n_params > REMD_CUSTOM_MAX_PARAMS || (d.n_params > 0 && !d.params))
        return "0 ... REMD_CUSTOM_MAX_PARAMS parameters per term are supported";
    return "";
}

// what custom_nonbonded.hip indexes unchecked: one parameter row per atom of the system, 2 n_params operands, the exclusion rows
inline std::string cst_check_nonbonded(const remd_custom_force_desc& d, const cst_facts& s)
{
    if (d.n_terms != s.N) return "a nonbonded force has " + std::to_string(d.n_terms) + " particles, the system has " + std::to_string(s.N);
    if (2 * d.n_params > REMD_CUSTOM_MAX_PARAMS) return "a nonbonded force takes at most REMD_CUSTOM_MAX_PARAMS / 2 per-particle parameters";
    if (d.nb_method < 0 || d.nb_method > 2) return "unknown nonbonded method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic)";
    if ((d.periodic != 0) != (d.nb_method == 2)) return "a nonbonded force is periodic exactly where its method is CutoffPeriodic";
    if (d.nb_method != 0 && !(d.cutoff > 0.0)) return "a cutoff that is not positive";
    if (d.switch_distance >= 0.0 && (d.nb_method == 0 || !(d.switch_distance > 0.0 && d.switch_distance < d.cutoff)))
        return "the switching distance must lie in (0, cutoff) and needs a cutoff";
    if (d.long_range_correction && d.nb_method != 2) return "a long-range correction needs CutoffPeriodic";
    if (!d.excl_offsets || d.excl_offsets[0] != 0) return "excl_offsets [N + 1] must start at 0";
    for (int a = 0; a < d.n_terms; ++a) {
        const int b = d.excl_offsets[a], e = d.excl_offsets[a + 1];
        if (e < b || (e > b && !d.excl_atoms)) return "excl_offsets must not decrease";
        for (int k = b; k < e; ++k) {
            if (d.excl_atoms[k] < 0 || d.excl_atoms[k] >= d.n_terms) return "exclusion index out of range";
            if (d.excl_atoms[k] == a) return "a particle excluded from itself";
        }
    }
    if (d.nb_method == 2)
        for (size_t k = 0; k < s.n_boxes; ++k) if (!(s.boxes[k] >= 2.0 * d.cutoff)) return "box smaller than twice the cutoff";
    return "";
}

// what custom_cv.hip indexes unchecked: the variables in CSR form, their particles, the reference beside them
inline std::string cst_check_cv(const remd_custom_force_desc& d, int N)
{
    if (d.n_terms != 1 || d.n_params != 0 || d.periodic != 0) return "a collective-variable force has n_terms = 1, no per-term parameters and is not periodic";
    if (d.n_cvs < 1 || d.n_cvs > REMD_CUSTOM_MAX_CVS) return "a collective-variable force has 1 ... REMD_CUSTOM_MAX_CVS collective variables";
    if (!d.cv_offsets || !d.cv_atoms || !d.cv_reference) return "a collective-variable force needs cv_offsets, cv_atoms and cv_reference";
    if (d.cv_offsets[0] != 0) return "cv_offsets must start at 0";
    std::vector<char> seen(N);
    for (int c = 0; c < d.n_cvs; ++c) {
        const std::string cv = "collective variable " + std::to_string(c) + ": ";
        const int b = d.cv_offsets[c], e = d.cv_offsets[c + 1];
        if (e < b || e - b < 3) return cv + "an RMSD needs at least 3 particles";
        std::fill(seen.begin(), seen.end(), 0);
        double m[3] = {0.0, 0.0, 0.0};
        for (int k = b; k < e; ++k) {
            const int a = d.cv_atoms[k];
            if (a < 0 || a >= N) return cv + "particle index out of range";
            if (seen[a]) return cv + "particle " + std::to_string(a) + " named twice";
            seen[a] = 1;
            for (int x = 0; x < 3; ++x) {
                if (!std::isfinite(d.cv_reference[3 * (size_t)k + x])) return cv + "a reference position that is not finite";
                m[x] += d.cv_reference[3 * (size_t)k + x];
            }
        }
        for (int x = 0; x < 3; ++x)
            if (!(fabs(m[x]) <= 1e-9 * (e - b))) return cv + "the reference must be centred on its own centroid (within 1e-9 nm)";
    }
    return "";
}

// what cmap.hip indexes unchecked: every term's map, every map's block (the header cst_table2d trusts, and its extent)
inline std::string cst_check_cmap(const remd_custom_force_desc& d)
{
    if (d.n_params != 0 || d.n_program != 0) return "a CMAP force has no per-term parameters and no program";
    if (d.n_maps < 1 || d.n_maps > REMD_CUSTOM_MAX_MAPS) return "a CMAP force has 1 ... REMD_CUSTOM_MAX_MAPS maps";
    if (!d.map_index || !d.map_offsets || !d.consts || d.n_consts <= 0) return "a CMAP force needs map_index, map_offsets and the maps' blocks in consts";
    for (int k = 0; k < d.n_terms; ++k)
        if (d.map_index[k] < 0 || d.map_index[k] >= d.n_maps) return "term " + std::to_string(k) + ": map index out of range";
    for (int m = 0; m < d.n_maps; ++m) {
        const std::string map = "map " + std::to_string(m) + ": ";
        const long long off = d.map_offsets[m];
        if (off < 0 || off + 8 > (long long)d.n_consts) return map + "a block that runs past n_consts";
        const double* B = d.consts + off;
        if (!(B[0] >= 3.0 && B[0] <= 256.0) || B[0] != floor(B[0]) || B[1] != B[0]) return map + "a block whose sizes are not nx = ny, an integer 3 ... 256";
        if (B[6] != 1.0) return map + "a block that is not periodic";
        if (B[2] != 0.0 || B[4] != 0.0 || !(fabs(B[3] - 2.0 * M_PI) <= 1e-12) || B[5] != B[3]) return map + "a block whose range is not [0, 2 pi] in both angles";
        const long long nn = (long long)B[0];
        if (off + 8 + 4 * nn * nn > (long long)d.n_consts) return map + "a block that runs past n_consts";
        for (long long k = 0; k < 4 * nn * nn; ++k) if (!std::isfinite(B[8 + k])) return map + "a node value that is not finite";
    }
    return "";
}

// what every descriptor of a call shares with the first, d0: the globals and the force group
inline std::string cst_check_shared(const remd_custom_force_desc& d, const remd_custom_force_desc& d0)
{
    if (d.n_globals != d0.n_globals) return "every descriptor must carry the handle's n_globals";
    for (int k = 0; k < d0.n_globals; ++k) if (d.global_defaults && d.global_defaults[k] != d0.global_defaults[k]) return "global_defaults differ between the descriptors";
    if (d.force_group != d0.force_group || d.force_group < 0 || d.force_group > 31)
        return "every custom force of a handle must sit in one force group (0 ... 31)";
    return "";
}

// a centroid force's groups: CSR offsets that start at 0 and increase (no empty group), atoms of the system, weights that sum to 1;
// and the group numbers its bonds name
inline std::string cst_check_groups(const remd_custom_force_desc& d, int N)
{
    if (d.n_groups <= 0 || !d.group_offsets || !d.group_atoms || !d.group_weights) return "a centroid-bond force needs n_groups > 0, group_offsets, group_atoms and group_weights";
    if (d.group_offsets[0] != 0) return "group_offsets must start at 0";
    for (int g = 0; g < d.n_groups; ++g) {
        const int b = d.group_offsets[g], e = d.group_offsets[g + 1];
        if (e <= b) return "group_offsets must increase (an empty group has no centroid)";
        double W = 0.0;
        for (int k = b; k < e; ++k) {
            if (d.group_atoms[k] < 0 || d.group_atoms[k] >= N) return "group atom index out of range";
            if (!(d.group_weights[k] >= 0.0)) return "negative group weight";
            W += d.group_weights[k];
        }
        if (!(fabs(W - 1.0) <= 1e-12)) return "the weights of a group must sum to 1 (within 1e-12)";
    }
    for (int k = 0; k < d.n_terms * d.n_particles; ++k) if (d.atoms[k] < 0 || d.atoms[k] >= d.n_groups) return "group index out of range";
    return "";
}

// one descriptor, in the order a caller has come to rely on: a descriptor with several faults reports the same first one
inline std::string cst_check_force(const remd_custom_force_desc& d, const remd_custom_force_desc& d0, const cst_facts& s)
{
    std::string bad = cst_check_shape(d);
    if (bad.empty() && d.kind == REMD_CUSTOM_NONBONDED) bad = cst_check_nonbonded(d, s);
    if (bad.empty() && d.kind == REMD_CUSTOM_CV) bad = cst_check_cv(d, s.N);
    if (bad.empty() && d.kind == REMD_CUSTOM_CMAP) bad = cst_check_cmap(d);
    if (bad.empty() && d.kind == REMD_CUSTOM_HBOND) bad = cst_check_hbond(d, s);
    if (bad.empty() && d.kind == REMD_CUSTOM_MANYPARTICLE) bad = cst_check_manyparticle(d, s);
    if (bad.empty()) bad = cst_check_shared(d, d0);
    if (bad.empty() && d.kind == REMD_CUSTOM_GB) bad = cst_check_gb(d, s);      // (with the programs of its stages, one by one)
    if (bad.empty() && d.kind != REMD_CUSTOM_CMAP && d.kind != REMD_CUSTOM_GB)   // (a CMAP force has no program)
        if (const char* p = check_program(d, cst_n_vars(d))) bad = p;
    if (bad.empty() && d.kind == REMD_CUSTOM_CENTROID) bad = cst_check_groups(d, s.N);
    if (bad.empty() && d.kind != REMD_CUSTOM_CENTROID)
        for (int k = 0; k < d.n_terms * cst_width(d); ++k) if (d.atoms[k] < 0 || d.atoms[k] >= s.N) return "atom index out of range";
    return bad;
}

// a checked descriptor's record, and its parameters, program, constants and kind-specific rows behind those of the forces before it
inline void cst_pack_force(const remd_custom_force_desc& d, const cst_facts& s, cst_plan& p)
{
    cst_force f{};
    f.kind = d.kind; f.periodic = d.periodic ? 1 : 0; f.n_terms = d.n_terms; f.n_params = d.n_params; f.n_particles = cst_width(d);
    f.npad = (d.n_terms + 63) / 64 * 64;
    f.par0 = (int)p.par.size(); f.prog0 = (int)p.prog.size() / 2; f.n_prog = d.n_program; f.const0 = (int)p.consts.size();
    f.switch_dist = -1.0;
    int par_stride = f.npad;
    if (d.kind == REMD_CUSTOM_NONBONDED) {
        // its wavefronts are the upper-triangular tiles of 64 x 64 atoms; its parameters one row per atom, [n_params][Npad]
        const int nb = (d.n_terms + 63) / 64;
        f.npad = 64 * (nb * (nb + 1) / 2);
        par_stride = s.Npad;
        f.nb_method = d.nb_method; f.cutoff = d.nb_method ? d.cutoff : 0.0; f.switch_dist = d.switch_distance >= 0.0 ? d.switch_distance : -1.0;
        f.lrc = d.long_range_correction ? 1 : 0;
        if (f.lrc) p.has_lrc = true;
        if (d.nb_method == 2) p.periodic_cutoff = std::max(p.periodic_cutoff, d.cutoff);
        f.excl0 = (int)p.excl_off.size();
        const int base = (int)p.excl_atoms.size();
        for (int a = 0; a <= d.n_terms; ++a) p.excl_off.push_back(base + d.excl_offsets[a]);
        if (d.excl_offsets[d.n_terms] > 0) p.excl_atoms.insert(p.excl_atoms.end(), d.excl_atoms, d.excl_atoms + d.excl_offsets[d.n_terms]);
    }
    if (d.kind == REMD_CUSTOM_HBOND) cst_pack_hbond(d, f, p);
    if (d.kind == REMD_CUSTOM_MANYPARTICLE) { cst_pack_manyparticle(d, s, f, p); par_stride = s.Npad; }
    if (d.kind == REMD_CUSTOM_GB) { cst_pack_gb(d, s, f, p); par_stride = s.Npad; }
    // parameters [n_params][npad]; a padding slot repeats the last term (finite arithmetic in lanes that add nothing)
    for (int q = 0; q < d.n_params; ++q) for (int k = 0; k < par_stride; ++k) p.par.push_back(d.params[(size_t)std::min(k, d.n_terms - 1) * d.n_params + q]);
    if (d.n_program > 0) p.prog.insert(p.prog.end(), d.program, d.program + 2 * (size_t)d.n_program);
    if (d.n_consts > 0) p.consts.insert(p.consts.end(), d.consts, d.consts + d.n_consts);
    if (d.kind == REMD_CUSTOM_CV) {
        // its variables join the handle's tables
        f.cv0 = p.n_cv; f.n_cvs = d.n_cvs;
        if (p.cv_off.empty()) p.cv_off.push_back(0);
        const int base = (int)p.cv_atoms.size(), total = d.cv_offsets[d.n_cvs];
        for (int c = 1; c <= d.n_cvs; ++c) p.cv_off.push_back(base + d.cv_offsets[c]);
        p.cv_atoms.insert(p.cv_atoms.end(), d.cv_atoms, d.cv_atoms + total);
        p.cv_ref.insert(p.cv_ref.end(), d.cv_reference, d.cv_reference + 3 * (size_t)total);
        p.n_cv += d.n_cvs;
    }
    if (d.kind == REMD_CUSTOM_CMAP) {
        // its maps join the handle's: each block's offset in the handle's constants
        f.map0 = (int)p.map_off.size(); f.n_maps = d.n_maps;
        for (int m = 0; m < d.n_maps; ++m) p.map_off.push_back(f.const0 + d.map_offsets[m]);
    }
    p.F.push_back(f);
}

// the padded term space: part by part (cst_part), within a part the forces in the descriptors' order
inline void cst_lay_out(cst_plan& p)
{
    for (int part = 0; part < CST_N_PARTS; ++part) {
        for (int i = 0; i < p.nf; ++i) {
            cst_force& f = p.F[i];
            if (cst_part_of_kind[f.kind] != part) continue;
            f.slot0 = p.total_pad; p.total_pad += f.npad;
            p.wave_force.insert(p.wave_force.end(), f.npad / 64, i);
        }
        p.part_end[part] = p.total_pad / 64;
    }
}

// the atoms of every slot; a centroid force's groups join the handle's group tables, and its rows hold the handle-wide group numbers
inline void cst_fill_atoms(const remd_custom_force_desc* desc, cst_plan& p)
{
    int rows = 4;
    for (const cst_force& f : p.F) rows = std::max(rows, f.n_particles);
    p.atoms.assign((size_t)rows * p.total_pad, 0);
    for (int i = 0; i < p.nf; ++i) {
        const cst_force& f = p.F[i]; const remd_custom_force_desc& d = desc[i];
        const int wd = f.n_particles, group0 = p.n_groups;       // (added to the atoms of a centroid force only)
        if (f.kind == REMD_CUSTOM_CENTROID) {
            if (p.grp_off.empty()) p.grp_off.push_back(0);
            for (int g = 0; g < d.n_groups; ++g) {
                p.grp_atoms.insert(p.grp_atoms.end(), d.group_atoms + d.group_offsets[g], d.group_atoms + d.group_offsets[g + 1]);
                p.grp_w.insert(p.grp_w.end(), d.group_weights + d.group_offsets[g], d.group_weights + d.group_offsets[g + 1]);
                p.grp_off.push_back((int)p.grp_atoms.size());
                p.grp_periodic.push_back(f.periodic);
            }
            p.n_groups += d.n_groups;
        }
        for (int s = 0; s < f.npad; ++s) for (int a = 0; a < wd; ++a)
            p.atoms[(size_t)a * p.total_pad + f.slot0 + s] = (f.kind == REMD_CUSTOM_CENTROID ? group0 : 0) + d.atoms[(size_t)std::min(s, f.n_terms - 1) * wd + a];
    }
}

// per group, every (bond, position) that names it, in table order: the spread kernel adds their gradients in this order
inline void cst_fill_refs(cst_plan& p)
{
    if (p.n_groups == 0) return;
    std::vector<std::vector<int>> named(p.n_groups);
    const int slot_c = p.begin(CST_CENTROID) * 64;
    for (const cst_force& f : p.F) {
        if (f.kind != REMD_CUSTOM_CENTROID) continue;
        for (int b = 0; b < f.n_terms; ++b) for (int a = 0; a < f.n_particles; ++a)
            named[p.atoms[(size_t)a * p.total_pad + f.slot0 + b]].push_back((f.slot0 + b - slot_c) * REMD_CUSTOM_MAX_PARTICLES + a);
    }
    p.ref_off.push_back(0);
    for (const std::vector<int>& v : named) { p.refs.insert(p.refs.end(), v.begin(), v.end()); p.ref_off.push_back((int)p.refs.size()); }
}

// the map of every slot of the CMAP forces' part (a padding slot repeats the last term's, like its atoms)
inline void cst_fill_map_index(const remd_custom_force_desc* desc, cst_plan& p)
{
    const int slot_m = p.begin(CST_CMAP) * 64;
    p.map_index.assign((size_t)p.end(CST_CMAP) * 64 - slot_m, 0);
    for (int i = 0; i < p.nf; ++i) {
        const cst_force& f = p.F[i];
        if (f.kind != REMD_CUSTOM_CMAP) continue;
        for (int s = 0; s < f.npad; ++s) p.map_index[f.slot0 + s - slot_m] = desc[i].map_index[std::min(s, f.n_terms - 1)];
    }
}

// no NonbondedForce and no built-in bonded term or constraint: the molecules a barostat scales are what the custom bonds, angles,
// torsions, compound bonds and CMAP terms join (OpenMM takes molecules from the bonds its forces report); the scaling kernels take
// contiguous ranges, so a molecule whose atoms are not one gives no table (the barostat then refuses)
inline void cst_fill_molecules(const remd_custom_force_desc* desc, int N, cst_plan& p)
{
    std::vector<int> root(N);
    for (int a = 0; a < N; ++a) root[a] = a;
    auto find = [&](int a) { while (root[a] != a) a = root[a] = root[root[a]]; return a; };
    for (int i = 0; i < p.nf; ++i) {
        const cst_force& f = p.F[i];
        if (f.kind == REMD_CUSTOM_HBOND) { cst_hbond_molecules(desc[i], f, find, root); continue; }
        if (f.kind == REMD_CUSTOM_EXTERNAL || f.kind == REMD_CUSTOM_CENTROID || f.kind == REMD_CUSTOM_NONBONDED || f.kind == REMD_CUSTOM_CV || f.kind == REMD_CUSTOM_MANYPARTICLE || f.kind == REMD_CUSTOM_GB) continue;
        for (int b = 0; b < f.n_terms; ++b) for (int a = 1; a < f.n_particles; ++a) {
            const int u = find(desc[i].atoms[(size_t)b * f.n_particles]), v = find(desc[i].atoms[(size_t)b * f.n_particles + a]);
            if (u != v) root[std::max(u, v)] = std::min(u, v);
        }
    }
    bool contiguous = true;                         // (roots are the lowest atom of a molecule: a range starts at its root)
    for (int a = 0; a < N && contiguous; ++a) {
        const int r = find(a);
        if (r == a) { p.mol_first.push_back(a); p.mol_size.push_back(1); }
        else if (r == p.mol_first.back()) p.mol_size.back()++;
        else contiguous = false;
    }
    if (!contiguous) { p.mol_first.clear(); p.mol_size.clear(); }
}

// The descriptors of one remd_set_custom_terms call (n > 0) -> `p`, filled, and an empty string; or the refusal, the sentence behind
// "remd_set_custom_terms: " (`p` then holds nothing of use).  Carries no state from call to call.
inline std::string cst_build_plan(const remd_custom_force_desc* desc, int n, const cst_facts& s, cst_plan& p)
{
    p = cst_plan();
    if (n > REMD_CUSTOM_MAX_FORCES) return "more than REMD_CUSTOM_MAX_FORCES custom forces";
    p.nf = n; p.ng = desc[0].n_globals;
    if (p.ng < 0 || p.ng > REMD_CUSTOM_MAX_GLOBALS) return "more than REMD_CUSTOM_MAX_GLOBALS global parameters";
    if (p.ng > 0 && !desc[0].global_defaults) return "global_defaults missing";
    p.defaults.assign(desc[0].global_defaults, desc[0].global_defaults + p.ng);
    for (int i = 0; i < n; ++i) {
        const std::string bad = cst_check_force(desc[i], desc[0], s);
        if (!bad.empty()) return "force " + std::to_string(i) + ": " + bad;
        cst_pack_force(desc[i], s, p);
    }
    cst_lay_out(p);
    cst_fill_atoms(desc, p);
    cst_fill_refs(p);
    cst_fill_map_index(desc, p);
    // every state starts from the defaults (remd_set_custom_globals replaces them)
    p.K = s.K; p.glob_version = s.states_version; p.uniform = true;
    for (int k = 0; k < std::max(s.K, 0); ++k) p.glob.insert(p.glob.end(), p.defaults.begin(), p.defaults.end());
    if (p.glob.empty()) p.glob.assign(1, 0.0);          // (a force without globals: the kernels still take a pointer)
    p.lrc.assign((size_t)std::max(s.K, 1) * n, 0.0);
    if (p.periodic_cutoff > 0.0 && s.bare) cst_fill_molecules(desc, s.N, p);
    return "";
}
