// The many-particle kind (REMD_CUSTOM_MANYPARTICLE, include/remd_hip_custom.h) in the host set-up of the custom forces: included by
// custom_plan.h behind the records it fills (cst_force, cst_plan, cst_facts), plain C++17 with no HIP header like it, so
// tools/custom_manyparticle_plan_check.cpp runs it under the host compiler's sanitizers (tests/test_custom_manyparticle_plan_cpu.py).
// custom_manyparticle.hip indexes the parameter table, the types and the exclusion rows unchecked, and searches a row by bisection:
// what a descriptor may name, and that every row is sorted, is settled here, once.
//
// The layout: a force's wavefronts in the padded term space are its central particles, one each: npad = 64 N, wavefront w of the force
// is particle w.  par holds its parameters [n_params][Npad] at par0 (one column per atom, a padding column repeats the last atom),
// REMD_CX_PARAM operand 3 q + s being parameter q of the particle in slot s; mp_types gains its types [Npad] (padding: the last
// atom's) at mp_types0; excl_off / excl_atoms gain its N + 1 row offsets (rebased) and its rows; mp_row0 is its first row among the
// handle's neighbour rows [mp_rows][REMD_CUSTOM_MP_MAX_NEIGHBORS] (Npad rows per such force, work buffers of cst_tables).
#pragma once

// what custom_manyparticle.hip indexes unchecked: one parameter row and one type per atom of the system, 3 n_params operands, the
// slots the program names, sorted exclusion rows
inline std::string cst_check_manyparticle(const remd_custom_force_desc& d, const cst_facts& s)
{
    if (d.n_terms != s.N) return "a many-particle force has " + std::to_string(d.n_terms) + " particles, the system has " + std::to_string(s.N);
    if (3 * d.n_params > REMD_CUSTOM_MAX_PARAMS) return "a many-particle force takes at most REMD_CUSTOM_MAX_PARAMS / 3 per-particle parameters";
    if (d.mp_permutation_mode < 0 || d.mp_permutation_mode > 1) return "unknown permutation mode (0 SinglePermutation, 1 UniqueCentralParticle)";
    if (d.mp_particle_mask < 0 || d.mp_particle_mask > 7) return "mp_particle_mask names the particle slots 0 ... 2";
    // the mask is exactly the slots the program names (check_program, later, settles everything else about the program)
    if (d.program && d.n_program > 0 && d.n_program <= REMD_CUSTOM_MAX_PROGRAM) {
        int named = 0;
        for (int pc = 0; pc < d.n_program; ++pc) {
            const int op = d.program[2 * pc], arg = d.program[2 * pc + 1];
            if (op < REMD_CX_DISTANCE || op > REMD_CX_DIHEDRAL) continue;
            for (int k = 0; k < op - REMD_CX_DISTANCE + 2; ++k) if (((arg >> (4 * k)) & 15) < 3) named |= 1 << ((arg >> (4 * k)) & 15);
        }
        if (named != d.mp_particle_mask) return "mp_particle_mask is not the set of particle slots the program names";
    }
    if (d.nb_method < 0 || d.nb_method > 2) return "unknown nonbonded method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic)";
    if ((d.periodic != 0) != (d.nb_method == 2)) return "a many-particle force is periodic exactly where its method is CutoffPeriodic";
    if (d.nb_method != 0 && !(d.cutoff > 0.0)) return "a cutoff that is not positive";
    if (d.nb_method == 0 && d.n_terms > REMD_CUSTOM_MP_MAX_NEIGHBORS + 1)
        return "a many-particle force without a cutoff takes at most REMD_CUSTOM_MP_MAX_NEIGHBORS + 1 particles";
    if (!d.mp_types) return "a many-particle force needs mp_types";
    for (int a = 0; a < d.n_terms; ++a) if (d.mp_types[a] < 0 || d.mp_types[a] > 31) return "particle " + std::to_string(a) + ": a type outside 0 ... 31";
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
    // symmetric: the neighbour search reads the row of the lower particle, the triplet stage the row of either
    for (int a = 0; a < d.n_terms; ++a)
        for (int k = d.excl_offsets[a]; k < d.excl_offsets[a + 1]; ++k) {
            const int o = d.excl_atoms[k];
            if (!std::binary_search(d.excl_atoms + d.excl_offsets[o], d.excl_atoms + d.excl_offsets[o + 1], a))
                return "particle " + std::to_string(a) + " excludes " + std::to_string(o) + ", which does not exclude it";
        }
    if (d.nb_method == 2)
        for (size_t k = 0; k < s.n_boxes; ++k) if (!(s.boxes[k] >= 2.0 * d.cutoff)) return "box smaller than twice the cutoff";
    return "";
}

// its record, types and exclusion rows behind those of the forces before it (cst_pack_force has set the common fields and appends
// the parameters [n_params][Npad] itself)
inline void cst_pack_manyparticle(const remd_custom_force_desc& d, const cst_facts& s, cst_force& f, cst_plan& p)
{
    f.npad = 64 * d.n_terms;                                   // one wavefront per central particle
    f.nb_method = d.nb_method; f.cutoff = d.nb_method ? d.cutoff : 0.0;
    if (d.nb_method == 2) p.periodic_cutoff = std::max(p.periodic_cutoff, d.cutoff);
    f.mp_mode = d.mp_permutation_mode; f.mp_mask = d.mp_particle_mask;
    for (int k = 0; k < 3; ++k) f.mp_filter[k] = d.mp_filter[k];
    f.mp_types0 = (int)p.mp_types.size();
    for (int k = 0; k < s.Npad; ++k) p.mp_types.push_back(d.mp_types[std::min(k, d.n_terms - 1)]);
    f.mp_row0 = p.mp_rows; p.mp_rows += s.Npad;
    f.excl0 = (int)p.excl_off.size();
    const int base = (int)p.excl_atoms.size();
    for (int a = 0; a <= d.n_terms; ++a) p.excl_off.push_back(base + d.excl_offsets[a]);
    if (d.excl_offsets[d.n_terms] > 0) p.excl_atoms.insert(p.excl_atoms.end(), d.excl_atoms, d.excl_atoms + d.excl_offsets[d.n_terms]);
}
