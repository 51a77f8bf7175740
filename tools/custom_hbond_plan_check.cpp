// The host set-up of the donor-acceptor forces (openmmtools_amd/csrc/custom_hbond_plan.h through custom_plan.h) in a stand-alone host
// program, meant to be built with the host compiler's sanitizers:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/custom_hbond_plan_check.cpp -o custom_hbond_plan_check
//     ./custom_hbond_plan_check CASE_FILE
//
// CASE_FILE (written by tests/test_custom_hbond_plan_cpu.py), little-endian: int32 number of cases; per case the facts of the handle (int32
// N, Npad, K, bare, n_boxes; int64 states_version; f64 boxes[n_boxes]), int32 n, then n REMD_CUSTOM_HBOND descriptors: 14 int32 (n_terms,
// n_params, n_program, n_consts, stack_depth, n_globals, periodic, force_group, nb_method, hb_n_donors, hb_n_acceptors, hb_n_donor_params,
// hb_n_acceptor_params, hb_particle_mask), 1 f64 (cutoff), then 9 arrays (program, consts, global_defaults, hb_donor_atoms,
// hb_acceptor_atoms, hb_donor_params, hb_acceptor_params, hb_excl_offsets, hb_excl_acceptors), each an int32 length (-1: a NULL pointer)
// and its elements.  Every array lives in a heap block of exactly its length, so a read past one is a sanitizer report.  Per case the
// program runs cst_build_plan on ONE plan object that all cases share and prints "REFUSED <sentence>" or "PLAN" and the members the
// donor-acceptor kind fills, one per line: name, count, values (f64 as %a).
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <memory>
#include "../openmmtools_amd/csrc/custom_plan.h"

static FILE* in;
template <class T> static T rd() { T v; if (fread(&v, sizeof(T), 1, in) != 1) { fprintf(stderr, "short case file\n"); exit(2); } return v; }
template <class T> static const T* rd_array(std::vector<std::unique_ptr<T[]>>& keep)
{
    const int len = rd<int32_t>();
    if (len < 0) return nullptr;
    keep.emplace_back(new T[len]);
    for (int k = 0; k < len; ++k) keep.back()[k] = rd<T>();
    return keep.back().get();
}
static void put(const char* name, const std::vector<int>& v) { printf("%s %zu", name, v.size()); for (int x : v) printf(" %d", x); printf("\n"); }
static void put(const char* name, const std::vector<double>& v) { printf("%s %zu", name, v.size()); for (double x : v) printf(" %a", x); printf("\n"); }

int main(int argc, char** argv)
{
    in = argc > 1 ? fopen(argv[1], "rb") : nullptr; if (!in) { fprintf(stderr, "usage: custom_hbond_plan_check CASE_FILE\n"); return 2; }
    const int n_cases = rd<int32_t>();
    cst_plan p;
    for (int c = 0; c < n_cases; ++c) {
        std::vector<std::unique_ptr<int32_t[]>> ki; std::vector<std::unique_ptr<double[]>> kd;
        cst_facts s{};
        s.N = rd<int32_t>(); s.Npad = rd<int32_t>(); s.K = rd<int32_t>(); s.bare = rd<int32_t>() != 0; s.n_boxes = rd<int32_t>();
        s.states_version = rd<int64_t>();
        std::vector<double> boxes(s.n_boxes); for (double& b : boxes) b = rd<double>();
        s.boxes = boxes.data();
        const int n = rd<int32_t>();
        std::vector<remd_custom_force_desc> D(n);
        for (remd_custom_force_desc& d : D) {
            d.kind = REMD_CUSTOM_HBOND; d.switch_distance = -1.0;
            d.n_terms = rd<int32_t>(); d.n_params = rd<int32_t>(); d.n_program = rd<int32_t>(); d.n_consts = rd<int32_t>();
            d.stack_depth = rd<int32_t>(); d.n_globals = rd<int32_t>(); d.periodic = rd<int32_t>(); d.force_group = rd<int32_t>();
            d.nb_method = rd<int32_t>(); d.hb_n_donors = rd<int32_t>(); d.hb_n_acceptors = rd<int32_t>(); d.hb_n_donor_params = rd<int32_t>();
            d.hb_n_acceptor_params = rd<int32_t>(); d.hb_particle_mask = rd<int32_t>();
            d.cutoff = rd<double>();
            // (a per-term table this kind must not have: given, zeroed, where a case asks for n_params > 0, so that the kind's own refusal is reached)
            if (d.n_params > 0 && d.n_terms > 0) { kd.emplace_back(new double[(size_t)d.n_params * d.n_terms]()); d.params = kd.back().get(); }
            d.program = rd_array(ki); d.consts = rd_array(kd); d.global_defaults = rd_array(kd);
            d.hb_donor_atoms = rd_array(ki); d.hb_acceptor_atoms = rd_array(ki); d.hb_donor_params = rd_array(kd); d.hb_acceptor_params = rd_array(kd);
            d.hb_excl_offsets = rd_array(ki); d.hb_excl_acceptors = rd_array(ki);
        }
        const std::string refusal = cst_build_plan(D.data(), n, s, p);
        if (!refusal.empty()) { printf("REFUSED %s\n", refusal.c_str()); continue; }
        printf("PLAN\n");
        printf("scalars 4 %d %d %d %d\n", p.nf, p.ng, p.K, p.total_pad);
        printf("periodic_cutoff 1 %a\n", p.periodic_cutoff);
        // (the parts up to the donor-acceptor one; the many-particle part behind it has tools/custom_manyparticle_plan_check.cpp)
        printf("part_end %d", (int)CST_HBOND + 1); for (int k = 0; k <= CST_HBOND; ++k) printf(" %d", p.end(k)); printf("\n");
        for (const cst_force& f : p.F)
            printf("force 15 %d %d %d %d %d %d %d %d %d %d %d %d %d %d %a\n", f.kind, f.periodic, f.n_terms, f.n_params, f.n_particles, f.slot0, f.npad,
                   f.par0, f.nb_method, f.excl0, f.hb_na, f.hb_atoms0, f.hb_npd * 100 + f.hb_npa, f.hb_mask, f.cutoff);
        put("wave_force", p.wave_force); put("hb_atoms", p.hb_atoms); put("par", p.par); put("excl_off", p.excl_off); put("excl_atoms", p.excl_atoms);
        put("map_index", p.map_index); put("mol_first", p.mol_first); put("mol_size", p.mol_size);
        printf("END\n");
    }
    return 0;
}
