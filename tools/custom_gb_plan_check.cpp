// The host set-up of the Generalized-Born forces (openmmtools_amd/csrc/custom_gb_plan.h through custom_plan.h) in a stand-alone host
// program, meant to be built with the host compiler's sanitizers:
//
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/custom_gb_plan_check.cpp -o custom_gb_plan_check
//     ./custom_gb_plan_check CASE_FILE
//
// CASE_FILE (written by tests/test_custom_gb_expr_cpu.py), little-endian: int32 number of cases; per case the facts of the handle
// (int32 N, Npad, K, n_boxes; f64 boxes[n_boxes]), then one REMD_CUSTOM_GB descriptor: 10 int32 (n_terms, n_params, n_program,
// n_consts, stack_depth, periodic, force_group, nb_method, gb_n_values, gb_n_stages), 1 f64 (cutoff), then 6 arrays (params, program,
// consts, excl_offsets, excl_atoms, gb_stages), each an int32 length (-1: a NULL pointer) and its elements.  Every array lives in a
// heap block of exactly its length, so a read past one is a sanitizer report.  Per case the program runs cst_build_plan on ONE plan
// object that all cases share and prints "REFUSED <sentence>" or "PLAN" and what the kind fills; "SLICES" lines give cst_gb_slices and
// the slice borders of a few particle counts.
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

int main(int argc, char** argv)
{
    in = argc > 1 ? fopen(argv[1], "rb") : nullptr; if (!in) { fprintf(stderr, "usage: custom_gb_plan_check CASE_FILE\n"); return 2; }
    for (int N : {1, 22, 64, 65, 130, 140, 2000, 5000}) {
        const int nb = (N + 63) / 64, s = cst_gb_slices(N);
        printf("SLICES %d %d %d", N, nb, s);
        for (int k = 0; k <= s; ++k) printf(" %d", cst_gb_slice_begin(nb, s, k));
        printf("\n");
    }
    const int n_cases = rd<int32_t>();
    cst_plan p;
    for (int c = 0; c < n_cases; ++c) {
        std::vector<std::unique_ptr<int32_t[]>> ki; std::vector<std::unique_ptr<double[]>> kd;
        cst_facts s{};
        s.N = rd<int32_t>(); s.Npad = rd<int32_t>(); s.K = rd<int32_t>(); s.n_boxes = rd<int32_t>(); s.bare = true; s.states_version = 1;
        std::vector<double> boxes(s.n_boxes); for (double& b : boxes) b = rd<double>();
        s.boxes = boxes.data();
        remd_custom_force_desc d = remd_custom_force_desc();
        d.kind = REMD_CUSTOM_GB; d.switch_distance = -1.0;
        d.n_terms = rd<int32_t>(); d.n_params = rd<int32_t>(); d.n_program = rd<int32_t>(); d.n_consts = rd<int32_t>();
        d.stack_depth = rd<int32_t>(); d.periodic = rd<int32_t>(); d.force_group = rd<int32_t>(); d.nb_method = rd<int32_t>();
        d.gb_n_values = rd<int32_t>(); d.gb_n_stages = rd<int32_t>();
        d.cutoff = rd<double>();
        d.params = rd_array(kd); d.program = rd_array(ki); d.consts = rd_array(kd);
        d.excl_offsets = rd_array(ki); d.excl_atoms = rd_array(ki); d.gb_stages = rd_array(ki);
        const std::string refusal = cst_build_plan(&d, 1, s, p);
        if (!refusal.empty()) { printf("REFUSED %s\n", refusal.c_str()); continue; }
        const cst_force& f = p.F[0];
        const cst_gb_work w = cst_gb_layout(s.Npad, f.gb_slices, f.gb_n_values);
        printf("PLAN\n");
        printf("scalars 4 %d %d %zu %d\n", p.nf, p.total_pad, p.gb_work, p.end(CST_GB) - p.begin(CST_GB));
        printf("force 9 %d %d %d %d %d %d %d %d %lld\n", f.kind, f.n_terms, f.npad, f.gb_n_values, f.gb_n_stages, f.gb_stage0, f.gb_slices, f.excl0, f.gb_work0);
        printf("layout 5 %zu %zu %zu %zu %zu\n", w.part, w.V, w.dV, w.dpart, w.total);
        printf("par 1 %zu\n", p.par.size());
        put("gb_stages", p.gb_stages); put("excl_off", p.excl_off); put("excl_atoms", p.excl_atoms);
        printf("END\n");
    }
    return 0;
}
