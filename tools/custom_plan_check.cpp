// The host set-up of the custom forces (openmmtools_amd/csrc/custom_plan.h) in a stand-alone host program, meant to be built with the
// host compiler's sanitizers:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/custom_plan_check.cpp -o custom_plan_check
//     ./custom_plan_check CASE_FILE
//
// CASE_FILE (written by tests/test_custom_plan_cpu.py), little-endian: int32 number of cases; per case the facts of the handle (int32 N,
// Npad, K, bare, n_boxes; int64 states_version; f64 boxes[n_boxes]), int32 n, then n descriptors: 15 int32 (kind, n_terms, n_params,
// n_program, n_consts, stack_depth, n_globals, periodic, force_group, n_particles, n_groups, nb_method, long_range_correction, n_cvs,
// n_maps), 2 f64 (cutoff, switch_distance), then the 15 arrays in the order of `arrays` below, each an int32 length (-1: a NULL
// pointer) and its elements.  Every array lives in a heap block of exactly its length, so a read past one is a sanitizer report.
// Per case the program runs cst_build_plan on ONE plan object that all cases share (a refusal must leave nothing behind that a later
// case could see) and prints "REFUSED <sentence>" or "PLAN" and the plan's members, one per line: name, count, values (f64 as %a).
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <memory>
#include "../openmmtools_amd/csrc/custom_plan.h"

static FILE* in;
template <class T> static T rd() { T v; if (fread(&v, sizeof(T), 1, in) != 1) { fprintf(stderr, "short case file\n"); exit(2); } return v; }
// an array of exactly `len` elements (len = 0: a block of no bytes, not NULL), or NULL for len = -1
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
    in = argc > 1 ? fopen(argv[1], "rb") : nullptr; if (!in) { fprintf(stderr, "usage: custom_plan_check CASE_FILE\n"); return 2; }
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
            d.kind = rd<int32_t>(); d.n_terms = rd<int32_t>(); d.n_params = rd<int32_t>(); d.n_program = rd<int32_t>(); d.n_consts = rd<int32_t>();
            d.stack_depth = rd<int32_t>(); d.n_globals = rd<int32_t>(); d.periodic = rd<int32_t>(); d.force_group = rd<int32_t>();
            d.n_particles = rd<int32_t>(); d.n_groups = rd<int32_t>(); d.nb_method = rd<int32_t>(); d.long_range_correction = rd<int32_t>();
            d.n_cvs = rd<int32_t>(); d.n_maps = rd<int32_t>();
            d.cutoff = rd<double>(); d.switch_distance = rd<double>();
            // `arrays`
            d.atoms = rd_array(ki); d.params = rd_array(kd); d.program = rd_array(ki); d.consts = rd_array(kd); d.global_defaults = rd_array(kd);
            d.group_offsets = rd_array(ki); d.group_atoms = rd_array(ki); d.group_weights = rd_array(kd);
            d.excl_offsets = rd_array(ki); d.excl_atoms = rd_array(ki);
            d.cv_offsets = rd_array(ki); d.cv_atoms = rd_array(ki); d.cv_reference = rd_array(kd);
            d.map_index = rd_array(ki); d.map_offsets = rd_array(ki);
        }
        const std::string refusal = cst_build_plan(D.data(), n, s, p);
        if (!refusal.empty()) { printf("REFUSED %s\n", refusal.c_str()); continue; }
        printf("PLAN\n");
        printf("scalars 10 %d %d %d %d %d %d %d %d %d %lld\n", p.nf, p.ng, p.K, p.total_pad, p.n_groups, p.n_cv, (int)p.uniform, (int)p.has_lrc,
               (int)p.lrc_valid, p.glob_version);
        printf("periodic_cutoff 1 %a\n", p.periodic_cutoff);
        // (the parts of the kinds this program can describe; the donor-acceptor part, the last one, has tools/custom_hbond_plan_check.cpp)
        printf("part_end %d", (int)CST_HBOND); for (int k = 0; k < CST_HBOND; ++k) printf(" %d", p.end(k)); printf("\n");
        printf("part_begin %d", (int)CST_HBOND); for (int k = 0; k < CST_HBOND; ++k) printf(" %d", p.begin(k)); printf("\n");
        for (const cst_force& f : p.F)
            printf("force 20 %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %a %a\n", f.kind, f.periodic, f.n_terms, f.n_params, f.n_particles,
                   f.slot0, f.npad, f.par0, f.prog0, f.n_prog, f.const0, f.nb_method, f.excl0, f.lrc, f.cv0, f.n_cvs, f.map0, f.n_maps, f.cutoff, f.switch_dist);
        put("wave_force", p.wave_force); put("atoms", p.atoms); put("par", p.par); put("consts", p.consts); put("glob", p.glob);
        put("defaults", p.defaults); put("prog", p.prog); put("grp_off", p.grp_off); put("grp_atoms", p.grp_atoms); put("grp_w", p.grp_w);
        put("grp_periodic", p.grp_periodic); put("ref_off", p.ref_off); put("refs", p.refs); put("cv_off", p.cv_off); put("cv_atoms", p.cv_atoms);
        put("cv_ref", p.cv_ref); put("map_off", p.map_off); put("map_index", p.map_index); put("excl_off", p.excl_off);
        put("excl_atoms", p.excl_atoms); put("lrc", p.lrc); put("mol_first", p.mol_first); put("mol_size", p.mol_size);
        printf("END\n");
    }
    return 0;
}
