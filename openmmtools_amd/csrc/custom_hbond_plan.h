// The donor-acceptor kind (REMD_CUSTOM_HBOND, include/remd_hip_custom.h) in the host set-up of the custom forces: included by custom_plan.h
// behind the records it fills (cst_force, cst_plan, cst_facts), plain C++17 with no HIP header like it, so tools/custom_hbond_plan_check.cpp
// runs it under the host compiler's sanitizers (tests/test_custom_hbond_plan_cpu.py).  custom_hbond.hip indexes the particle tables, the
// two parameter tables and the exclusion rows unchecked: what a descriptor may name is settled here, once.
//
// The layout: a force's wavefronts are its tiles of 64 donors x 64 acceptors, ALL of them, row by row: tile t of the force is donor block
// t / nbA and acceptor block t % nbA, nbA = ceil(nA / 64); npad = 64 ceil(nD / 64) nbA.  hb_atoms holds per force the donors' particles
// [3][ndpad], then the acceptors' [3][napad]; par the donors' parameters [hb_npd][ndpad] at par0, then the acceptors' [hb_npa][napad];
// every padding column repeats its side's last row; excl_off / excl_atoms gain the force's hb_n_donors + 1 row offsets (rebased) and its
// acceptor indices.
#pragma once

// what custom_hbond.hip indexes unchecked: the particles of every donor and acceptor, the particle slots the program names, the two
// parameter tables, the exclusion rows
inline std::string cst_check_hbond(const remd_custom_force_desc& d, const cst_facts& s)
{
    if (d.hb_n_donors != d.n_terms || d.hb_n_acceptors <= 0) return "a donor-acceptor force has n_terms = hb_n_donors > 0 and hb_n_acceptors > 0";
    if (d.n_params != 0 || d.params) return "a donor-acceptor force has n_params = 0 (its parameters are hb_donor_params and hb_acceptor_params)";
    if (!d.hb_donor_atoms || !d.hb_acceptor_atoms) return "a donor-acceptor force needs hb_donor_atoms and hb_acceptor_atoms";
    if (d.hb_n_donor_params < 0 || d.hb_n_acceptor_params < 0 || d.hb_n_donor_params + d.hb_n_acceptor_params > REMD_CUSTOM_MAX_PARAMS)
        return "a donor-acceptor force takes at most REMD_CUSTOM_MAX_PARAMS per-donor and per-acceptor parameters together";
    if ((d.hb_n_donor_params > 0 && !d.hb_donor_params) || (d.hb_n_acceptor_params > 0 && !d.hb_acceptor_params)) return "a parameter table is missing";
    if (d.hb_particle_mask < 0 || d.hb_particle_mask > 63) return "hb_particle_mask names the particle slots 0 ... 5";
    // the mask is exactly the slots the program names (check_program, later, settles everything else about the program)
    if (d.program && d.n_program > 0 && d.n_program <= REMD_CUSTOM_MAX_PROGRAM) {
        int named = 0;
        for (int pc = 0; pc < d.n_program; ++pc) {
            const int op = d.program[2 * pc], arg = d.program[2 * pc + 1];
            if (op < REMD_CX_DISTANCE || op > REMD_CX_DIHEDRAL) continue;
            for (int k = 0; k < op - REMD_CX_DISTANCE + 2; ++k) if (((arg >> (4 * k)) & 15) < 6) named |= 1 << ((arg >> (4 * k)) & 15);
        }
        if (named != d.hb_particle_mask) return "hb_particle_mask is not the set of particle slots the program names";
    }
    if (d.nb_method < 0 || d.nb_method > 2) return "unknown nonbonded method (0 NoCutoff, 1 CutoffNonPeriodic, 2 CutoffPeriodic)";
    if ((d.periodic != 0) != (d.nb_method == 2)) return "a donor-acceptor force is periodic exactly where its method is CutoffPeriodic";
    if (d.nb_method != 0 && !(d.cutoff > 0.0)) return "a cutoff that is not positive";
    for (int side = 0; side < 2; ++side) {
        const int n = side ? d.hb_n_acceptors : d.hb_n_donors;
        const int32_t* A = side ? d.hb_acceptor_atoms : d.hb_donor_atoms;
        const std::string who = side ? "acceptor " : "donor ";
        for (int i = 0; i < n; ++i) for (int q = 0; q < 3; ++q) {
            const int a = A[3 * (size_t)i + q];
            if (a < -1 || a >= s.N) return who + std::to_string(i) + ": atom index out of range";
            if (a < 0 && q == 0) return who + std::to_string(i) + ": the first particle is missing";
            if (a < 0 && ((d.hb_particle_mask >> (3 * side + q)) & 1)) return who + std::to_string(i) + ": the program names a particle it does not have";
            for (int k = 0; k < q; ++k) if (a >= 0 && A[3 * (size_t)i + k] == a) return who + std::to_string(i) + ": atom " + std::to_string(a) + " named twice";
        }
    }
    if (!d.hb_excl_offsets || d.hb_excl_offsets[0] != 0) return "hb_excl_offsets [hb_n_donors + 1] must start at 0";
    std::vector<char> excluded(d.hb_n_acceptors);
    for (int i = 0; i < d.hb_n_donors; ++i) {
        const int b = d.hb_excl_offsets[i], e = d.hb_excl_offsets[i + 1];
        if (e < b || (e > b && !d.hb_excl_acceptors)) return "hb_excl_offsets must not decrease";
        std::fill(excluded.begin(), excluded.end(), 0);
        for (int k = b; k < e; ++k) {
            const int a = d.hb_excl_acceptors[k];
            if (a < 0 || a >= d.hb_n_acceptors) return "exclusion index out of range";
            if (excluded[a]) return "donor " + std::to_string(i) + " excludes acceptor " + std::to_string(a) + " twice";
            if (k > b && d.hb_excl_acceptors[k - 1] > a) return "an exclusion row that is not sorted";
            excluded[a] = 1;
        }
        // a pair that shares a particle has no geometry of its own
        for (int j = 0; j < d.hb_n_acceptors; ++j) {
            if (excluded[j]) continue;
            for (int q = 0; q < 3; ++q) for (int k = 0; k < 3; ++k)
                if (d.hb_donor_atoms[3 * (size_t)i + q] >= 0 && d.hb_donor_atoms[3 * (size_t)i + q] == d.hb_acceptor_atoms[3 * (size_t)j + k])
                    return "donor " + std::to_string(i) + " and acceptor " + std::to_string(j) + " share atom " + std::to_string(d.hb_donor_atoms[3 * (size_t)i + q]) + " and are not excluded";
        }
    }
    if (d.nb_method == 2)
        for (size_t k = 0; k < s.n_boxes; ++k) if (!(s.boxes[k] >= 2.0 * d.cutoff)) return "box smaller than twice the cutoff";
    return "";
}


// its record, particles, parameters and exclusion rows behind those of the forces before it (cst_pack_force has set the common fields)
inline void cst_pack_hbond(const remd_custom_force_desc& d, cst_force& f, cst_plan& p)
{
    // its wavefronts are the tiles of 64 donors x 64 acceptors, row by row; particles and parameters one column per donor, then
    // per acceptor, each side padded to whole blocks with its last row repeated
    const int nd = d.hb_n_donors, na = d.hb_n_acceptors, ndpad = (nd + 63) / 64 * 64, napad = (na + 63) / 64 * 64;
    f.npad = (ndpad / 64) * napad;
    f.hb_na = na; f.hb_npd = d.hb_n_donor_params; f.hb_npa = d.hb_n_acceptor_params; f.hb_mask = d.hb_particle_mask;
    f.nb_method = d.nb_method; f.cutoff = d.nb_method ? d.cutoff : 0.0;
    if (d.nb_method == 2) p.periodic_cutoff = std::max(p.periodic_cutoff, d.cutoff);
    f.hb_atoms0 = (int)p.hb_atoms.size();
    for (int q = 0; q < 3; ++q) for (int k = 0; k < ndpad; ++k) p.hb_atoms.push_back(d.hb_donor_atoms[3 * (size_t)std::min(k, nd - 1) + q]);
    for (int q = 0; q < 3; ++q) for (int k = 0; k < napad; ++k) p.hb_atoms.push_back(d.hb_acceptor_atoms[3 * (size_t)std::min(k, na - 1) + q]);
    for (int q = 0; q < f.hb_npd; ++q) for (int k = 0; k < ndpad; ++k) p.par.push_back(d.hb_donor_params[(size_t)std::min(k, nd - 1) * f.hb_npd + q]);
    for (int q = 0; q < f.hb_npa; ++q) for (int k = 0; k < napad; ++k) p.par.push_back(d.hb_acceptor_params[(size_t)std::min(k, na - 1) * f.hb_npa + q]);
    f.excl0 = (int)p.excl_off.size();
    const int base = (int)p.excl_atoms.size();
    for (int a = 0; a <= nd; ++a) p.excl_off.push_back(base + d.hb_excl_offsets[a]);
    if (d.hb_excl_offsets[nd] > 0) p.excl_atoms.insert(p.excl_atoms.end(), d.hb_excl_acceptors, d.hb_excl_acceptors + d.hb_excl_offsets[nd]);
}

// the atoms a barostat must move together (cst_fill_molecules): a donor's particles, and an acceptor's
template <class Find>
inline void cst_hbond_molecules(const remd_custom_force_desc& d, const cst_force& f, Find&& find, std::vector<int>& root)
{
    for (int side = 0; side < 2; ++side) {
        const int32_t* A = side ? d.hb_acceptor_atoms : d.hb_donor_atoms;
        for (int b = 0; b < (side ? f.hb_na : f.n_terms); ++b) for (int a = 1; a < 3; ++a) {
            if (A[3 * (size_t)b + a] < 0) continue;
            const int u = find(A[3 * (size_t)b]), v = find(A[3 * (size_t)b + a]);
            if (u != v) root[std::max(u, v)] = std::min(u, v);
        }
    }
}
