// The Generalized-Born kind (REMD_CUSTOM_GB, include/remd_hip_custom.h) in the host set-up of the custom forces: included by
// custom_plan.h behind the records it fills (cst_force, cst_plan, cst_facts) and behind check_program, plain C++17 with no HIP header
// like it, so tools/custom_gb_plan_check.cpp runs it under the host compiler's sanitizers (tests/test_custom_gb_expr_cpu.py).
// custom_gb.hip indexes the stage table, the parameter table, the value and partial-sum buffers and the exclusion rows unchecked: what
// a descriptor may name is settled here, once.
//
// The layout: with nb = ceil(N / 64) row blocks and `slices` column slices (cst_gb_slices), the force's wavefronts in the padded term
// space are nb slices tiles of the pair-term launch, row block by row block, then nb wavefronts of the per-particle launch:
// npad = 64 nb (slices + 1); those are the slots its energies land in.  par holds its parameters [n_params][Npad] at par0; gb_stages
// gains its rows at gb_stage0; excl_off / excl_atoms gain its N + 1 row offsets (rebased) and its rows.  Its work buffers are doubles
// per replica, gb_work0 the force's first (cst_gb_work lays them out; Npad doubles each):
//     part [slices]        value 0 in partial sums per slice                                (launch 1 -> 2)
//     V    [n_values]      the values                                                       (launch 2 -> 3, 4, 5)
//     dV   [n_values]      dE/dV_k of the single-particle terms; [0] ends as dE/dV_0        (launch 2 -> 4 -> 5)
//     dpart[slices][n_values]  dE/dV_k of the pair terms in partial sums per slice          (launch 3 -> 4)
#pragma once

enum { CGB_TYPE = 0, CGB_EXCL, CGB_TARGET, CGB_PASS, CGB_PROG0, CGB_NPROG, CGB_DEPTH, CGB_VAR0, CGB_NCOLS = 10, CGB_COL0 = 11 };
enum { CGB_PAIR_VALUE = 0, CGB_SINGLE_VALUE, CGB_SINGLE_ENERGY, CGB_PAIR_ENERGY };

// the wavefronts one replica's pair launch should at least have: with 8 replicas of 2000 particles (32 row blocks) two slices, 512
// wavefronts on the 256 compute units of an MI355X
#define REMD_CUSTOM_GB_WAVES_PER_REPLICA 64

// column slices of a force of N particles: enough for REMD_CUSTOM_GB_WAVES_PER_REPLICA wavefronts, at most one per column block
inline int cst_gb_slices(int N)
{
    const int nb = (N + 63) / 64;
    return std::max(1, std::min(nb, (REMD_CUSTOM_GB_WAVES_PER_REPLICA + nb - 1) / nb));
}
// (the two functions the kernels share with the host: the host compiler sees no qualifier)
#ifdef __HIPCC__
#define CST_GB_HD __host__ __device__
#else
#define CST_GB_HD
#endif
// the column blocks [begin, end) of slice s
CST_GB_HD inline int cst_gb_slice_begin(int nb, int slices, int s) { return (int)((long long)s * nb / slices); }

struct cst_gb_work { size_t part, V, dV, dpart, total; };       // offsets in doubles within the force's share of one replica
CST_GB_HD inline cst_gb_work cst_gb_layout(int Npad, int slices, int n_values)
{
    cst_gb_work w;
    w.part = 0;
    w.V = w.part + (size_t)slices * Npad;
    w.dV = w.V + (size_t)n_values * Npad;
    w.dpart = w.dV + (size_t)n_values * Npad;
    w.total = w.dpart + (size_t)slices * n_values * Npad;
    return w;
}

// a quantity code of stage type `type` that may name values below `values_known` and parameters below n_params
inline bool cst_gb_quantity_ok(int code, int type, int values_known, int n_params, bool differentiated)
{
    const bool pair = type == CGB_PAIR_VALUE || type == CGB_PAIR_ENERGY;
    if (code == 0) return pair;
    if (code >= 1 && code < 1 + 2 * REMD_CUSTOM_GB_MAX_VALUES) return (code - 1) / 2 < values_known && (pair || ((code - 1) & 1) == 0);
    if (code >= 16 && code < 16 + 2 * REMD_CUSTOM_MAX_PARAMS) return !differentiated && (code - 16) / 2 < n_params && (pair || ((code - 16) & 1) == 0);
    return false;
}

// what custom_gb.hip indexes unchecked: one parameter row per atom, the stage table and every stage's program, the exclusion rows
inline std::string cst_check_gb(const remd_custom_force_desc& d, const cst_facts& s)
{
    if (d.n_terms != s.N) return "a Generalized-Born force has " + std::to_string(d.n_terms) + " particles, the system has " + std::to_string(s.N);
    if (d.nb_method < 0 || d.nb_method > 2) return "unknown nonbonded method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic)";
    if ((d.periodic != 0) != (d.nb_method == 2)) return "a Generalized-Born force is periodic exactly where its method is CutoffPeriodic";
    if (d.nb_method != 0 && !(d.cutoff > 0.0)) return "a cutoff that is not positive";
    if (!d.excl_offsets || d.excl_offsets[0] != 0) return "excl_offsets [N + 1] must start at 0";
    for (int a = 0; a < d.n_terms; ++a) {
        const int b = d.excl_offsets[a], e = d.excl_offsets[a + 1];
        if (e < b || (e > b && !d.excl_atoms)) return "excl_offsets must not decrease";
        for (int k = b; k < e; ++k) {
            if (d.excl_atoms[k] < 0 || d.excl_atoms[k] >= d.n_terms) return "exclusion index out of range";
            if (d.excl_atoms[k] == a) return "a particle excluded from itself";
            if (k > b && d.excl_atoms[k - 1] >= d.excl_atoms[k]) return "an exclusion row that is not sorted, or names a particle twice";
        }
    }
    for (int a = 0; a < d.n_terms; ++a)
        for (int k = d.excl_offsets[a]; k < d.excl_offsets[a + 1]; ++k) {
            const int o = d.excl_atoms[k];
            if (!std::binary_search(d.excl_atoms + d.excl_offsets[o], d.excl_atoms + d.excl_offsets[o + 1], a))
                return "particle " + std::to_string(a) + " excludes " + std::to_string(o) + ", which does not exclude it";
        }
    if (d.nb_method == 2)
        for (size_t k = 0; k < s.n_boxes; ++k) if (!(s.boxes[k] >= 2.0 * d.cutoff)) return "box smaller than twice the cutoff";
    if (d.gb_n_values < 1 || d.gb_n_values > REMD_CUSTOM_GB_MAX_VALUES) return "a Generalized-Born force has 1 ... REMD_CUSTOM_GB_MAX_VALUES computed values";
    if (d.gb_n_stages < 1 || d.gb_n_stages > REMD_CUSTOM_GB_MAX_STAGES || !d.gb_stages) return "a Generalized-Born force has 1 ... REMD_CUSTOM_GB_MAX_STAGES stages";
    if (d.n_program <= 0 || !d.program) return "an empty program";
    int values_known = 0; bool energies = false, term_seen[REMD_CUSTOM_GB_MAX_TERMS] = {};
    for (int k = 0; k < d.gb_n_stages; ++k) {
        const int32_t* g = d.gb_stages + (size_t)k * REMD_CUSTOM_GB_STAGE_INTS;
        const std::string stage = "stage " + std::to_string(k) + ": ";
        const int type = g[CGB_TYPE];
        if (type < CGB_PAIR_VALUE || type > CGB_PAIR_ENERGY) return stage + "unknown type";
        if ((k == 0) != (type == CGB_PAIR_VALUE)) return stage + "the pair value is stage 0 and the only one of its type";
        if (g[CGB_EXCL] != 0 && g[CGB_EXCL] != 1) return stage + "the exclusion flag is 0 or 1";
        const bool value = type == CGB_PAIR_VALUE || type == CGB_SINGLE_VALUE;
        if (value) {
            if (energies) return stage + "a value behind an energy term";
            if (g[CGB_TARGET] != values_known || values_known >= d.gb_n_values) return stage + "the values come in order, gb_n_values of them";
            if (g[CGB_PASS] != 0) return stage + "a value has one pass";
        } else {
            energies = true;
            if (values_known != d.gb_n_values) return stage + "an energy term in front of a value";
            if (g[CGB_TARGET] < 0 || g[CGB_TARGET] >= REMD_CUSTOM_GB_MAX_TERMS) return stage + "a Generalized-Born force has at most REMD_CUSTOM_GB_MAX_TERMS energy terms";
            if (g[CGB_PASS] < 0 || g[CGB_PASS] > 2) return stage + "pass out of range";
            if ((g[CGB_PASS] == 0) == term_seen[g[CGB_TARGET]]) return stage + "the passes of an energy term start at 0, once";
            term_seen[g[CGB_TARGET]] = true;
        }
        int n_vars = 0;
        for (int v = 0; v < 3; ++v) {
            const int code = g[CGB_VAR0 + v];
            if (code == -1) continue;
            if (n_vars != v) return stage + "the variables are the first ones";
            if (!cst_gb_quantity_ok(code, type, values_known, d.n_params, true)) return stage + "a variable that is not r or a value known to the stage";
            n_vars = v + 1;
        }
        if (type == CGB_PAIR_VALUE && (n_vars != 1 || g[CGB_VAR0] != 0)) return stage + "the pair value has the one variable r";
        if (g[CGB_NCOLS] < 0 || g[CGB_NCOLS] > REMD_CUSTOM_MAX_PARAMS) return stage + "a program that names more than REMD_CUSTOM_MAX_PARAMS staged columns";
        for (int c = 0; c < g[CGB_NCOLS]; ++c)
            if (!cst_gb_quantity_ok(g[CGB_COL0 + c], type, values_known, d.n_params, false)) return stage + "a staged column that is no quantity of the stage";
        if (g[CGB_PROG0] < 0 || g[CGB_NPROG] <= 0 || (long long)g[CGB_PROG0] + g[CGB_NPROG] > (long long)d.n_program) return stage + "a program outside the force's";
        // the stage's program as one of its own: the variables and the staged columns are what it may name, no globals
        remd_custom_force_desc sub = d;
        sub.kind = REMD_CUSTOM_BOND; sub.program = d.program + 2 * (size_t)g[CGB_PROG0]; sub.n_program = g[CGB_NPROG];
        sub.stack_depth = g[CGB_DEPTH]; sub.n_params = g[CGB_NCOLS]; sub.n_globals = 0;
        if (const char* bad = check_program(sub, n_vars)) return stage + bad;
        if (value) ++values_known;
    }
    if (values_known != d.gb_n_values) return "the stage table holds fewer values than gb_n_values";
    return "";
}

// its record, stage rows and exclusion rows behind those of the forces before it (cst_pack_force has set the common fields and appends
// the parameters [n_params][Npad], the program and the constants itself)
inline void cst_pack_gb(const remd_custom_force_desc& d, const cst_facts& s, cst_force& f, cst_plan& p)
{
    const int nb = (d.n_terms + 63) / 64;
    f.gb_slices = cst_gb_slices(d.n_terms);
    f.npad = 64 * nb * (f.gb_slices + 1);
    f.nb_method = d.nb_method; f.cutoff = d.nb_method ? d.cutoff : 0.0;
    if (d.nb_method == 2) p.periodic_cutoff = std::max(p.periodic_cutoff, d.cutoff);
    f.gb_n_values = d.gb_n_values; f.gb_n_stages = d.gb_n_stages;
    f.gb_stage0 = (int)p.gb_stages.size() / REMD_CUSTOM_GB_STAGE_INTS;
    p.gb_stages.insert(p.gb_stages.end(), d.gb_stages, d.gb_stages + (size_t)d.gb_n_stages * REMD_CUSTOM_GB_STAGE_INTS);
    f.gb_work0 = (long long)p.gb_work;
    p.gb_work += cst_gb_layout(s.Npad, f.gb_slices, d.gb_n_values).total;
    f.excl0 = (int)p.excl_off.size();
    const int base = (int)p.excl_atoms.size();
    for (int a = 0; a <= d.n_terms; ++a) p.excl_off.push_back(base + d.excl_offsets[a]);
    if (d.excl_offsets[d.n_terms] > 0) p.excl_atoms.insert(p.excl_atoms.end(), d.excl_atoms, d.excl_atoms + d.excl_offsets[d.n_terms]);
}
