// The host set-up of the many-particle forces (openmmtools_amd/csrc/custom_manyparticle_plan.h through custom_plan.h) in a stand-alone
// host program, meant to be built with the host compiler's sanitizers:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/custom_manyparticle_plan_check.cpp -o custom_manyparticle_plan_check
//     ./custom_manyparticle_plan_check CASE_FILE
//
// CASE_FILE (written by tests/test_custom_manyparticle_plan_cpu.py), little-endian: int32 number of cases; per case the facts of the
// handle (int32 N, Npad, K, bare, n_boxes; int64 states_version; f64 boxes[n_boxes]), int32 n, then n REMD_CUSTOM_MANYPARTICLE
// descriptors: 14 int32 (n_terms, n_params, n_program, n_consts, stack_depth, n_globals, periodic, force_group, nb_method,
// mp_permutation_mode, mp_particle_mask, mp_filter[0 ... 2]), 1 f64 (cutoff), then 7 arrays (params, program, consts, global_defaults,
// mp_types, excl_offsets, excl_atoms), each an int32 length (-1: a NULL pointer) and its elements.  Every array lives in a heap block of
// exactly its length, so a read past one is a sanitizer report.  Per case the program runs cst_build_plan on ONE plan object that all
// cases share and prints "REFUSED <sentence>" or "PLAN" and the members the many-particle kind fills, one per line: name, count, values
// (f64 as %a).
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
    in = argc > 1 ? fopen(argv[1], "rb") : nullptr; if (!in) { fprintf(stderr, "usage: custom_manyparticle_plan_check CASE_FILE\n"); return 2; }
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
            d = remd_custom_force_desc();
            d.kind = REMD_CUSTOM_MANYPARTICLE; d.switch_distance = -1.0;
            d.n_terms = rd<int32_t>(); d.n_params = rd<int32_t>(); d.n_program = rd<int32_t>(); d.n_consts = rd<int32_t>();
            d.stack_depth = rd<int32_t>(); d.n_globals = rd<int32_t>(); d.periodic = rd<int32_t>(); d.force_group = rd<int32_t>();
            d.nb_method = rd<int32_t>(); d.mp_permutation_mode = rd<int32_t>(); d.mp_particle_mask = rd<int32_t>();
            for (int k = 0; k < 3; ++k) d.mp_filter[k] = (uint32_t)rd<int32_t>();
            d.cutoff = rd<double>();
            d.params = rd_array(kd); d.program = rd_array(ki); d.consts = rd_array(kd); d.global_defaults = rd_array(kd);
            d.mp_types = rd_array(ki); d.excl_offsets = rd_array(ki); d.excl_atoms = rd_array(ki);
        }
        const std::string refusal = cst_build_plan(D.data(), n, s, p);
        if (!refusal.empty()) { printf("REFUSED %s\n", refusal.c_str()); continue; }
        printf("PLAN\n");
        printf("scalars 5 %d %d %d %d %d\n", p.nf, p.ng, p.K, p.total_pad, p.mp_rows);
        printf("periodic_cutoff 1 %a\n", p.periodic_cutoff);
        printf("part_end %d", (int)CST_MANYPARTICLE + 1); for (int k = 0; k <= CST_MANYPARTICLE; ++k) printf(" %d", p.end(k)); printf("\n");   // (the parts up to this kind's: later kinds add theirs behind it)
        for (const cst_force& f : p.F)
            printf("force 17 %d %d %d %d %d %d %d %d %d %d %d %d %d %u %u %u %a\n", f.kind, f.periodic, f.n_terms, f.n_params, f.slot0, f.npad,
                   f.par0, f.nb_method, f.excl0, f.mp_mode, f.mp_types0, f.mp_row0, f.mp_mask, f.mp_filter[0], f.mp_filter[1], f.mp_filter[2], f.cutoff);
        put("wave_force", p.wave_force); put("mp_types", p.mp_types); put("par", p.par); put("excl_off", p.excl_off); put("excl_atoms", p.excl_atoms);
        put("mol_first", p.mol_first); put("mol_size", p.mol_size);
        printf("END\n");
    }
    return 0;
}
