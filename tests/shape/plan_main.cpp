// plan_main.cpp -- carma_shape_plan.h (which kernel a call runs) as a stand-alone program; test harness.  It can run under the host
// sanitizers (g++ -fsanitize=address,undefined); tests/test_shape_plan_cpu.py builds and runs it plain.
// One case per line on stdin, one plan per line on stdout.  SW: the thirteen switches in the order of ShapeSwitches, "u" for unset.
//   ld   p B n flags cus lpc_blocks SW          -> ld shape p G repeated_dt sl ho fold unrolled pairs waves rot grid block name
//   car1 B n cus SW                             -> ld ... (the same fields)
//   fam  p T R n cus row_per_cu force lane_min SW   -> fam family capacity        (force: 0 none, 1 ladder, 2 row, 3 lane)
//   row  R T T_global n flags cus lds_global SW -> row two win minw ho sl wpl grid rot xcd_map cooperative pipeline
//   lad  p d T R n cus ring_bytes SW            -> lad fits_pc nthr_fit lds_fit pc maxt nthr lds
//   flags p max_freq n t[n]                     -> flags word
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../carma_pack_amd/csrc/carma_shape_plan.h"

using namespace carma;

static long num(std::istringstream& in)
{
    std::string w;
    if (!(in >> w)) {
        fprintf(stderr, "plan_main: a value is missing\n");
        exit(2);
    }
    return w == "u" ? TUNE_UNSET : atol(w.c_str());
}

static ShapeSwitches switches(std::istringstream& in)
{
    ShapeSwitches sw;
    long* const f[13] = {&sw.win_rows, &sw.win2_evals, &sw.pt_row_win, &sw.p3l_rows, &sw.lane_min, &sw.lpc_min, &sw.lpc_max, &sw.lpc_rot,
                         &sw.car1_scan_max, &sw.pt_row_wgs_per_cu, &sw.pt_row_rot, &sw.pt_row_xcd_map, &sw.pt_plain};
    for (long* v : f) *v = num(in);
    return sw;
}

static void put_ld(const LdPlan& pl)
{
    char name[128];
    if (logdens_plan_name(pl, name, sizeof(name)) <= 0) exit(3);
    printf("ld %d %d %d %d %d %d %d %d %d %d %d %ld %d %s\n", (int)pl.shape, pl.p, pl.G, (int)pl.repeated_dt, (int)pl.sl, (int)pl.ho, (int)pl.fold,
           (int)pl.unrolled, pl.pairs, pl.waves, pl.rot, pl.grid, pl.block, name);
}

int main()
{
    std::string line, mode;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> mode)) continue;
        if (mode == "ld") {
            const int p = (int)num(in);
            const long B = num(in);
            const int n = (int)num(in), flags = (int)num(in);
            DeviceFacts f;
            f.cus = (int)num(in), f.lpc_blocks = (int)num(in);
            put_ld(logdens_plan(p, B, n, flags, f, switches(in)));
        } else if (mode == "car1") {
            const long B = num(in);
            const int n = (int)num(in), cus = (int)num(in);
            put_ld(logdens_plan_car1(B, n, cus, switches(in)));
        } else if (mode == "fam") {
            const int p = (int)num(in), T = (int)num(in);
            const long R = num(in);
            const int n = (int)num(in);
            DeviceFacts f;
            f.cus = (int)num(in), f.row_per_cu = (int)num(in);
            const PtForce force = (PtForce)num(in);
            const long lane_min = num(in);
            const ShapeSwitches sw = switches(in);
            printf("fam %d %ld\n", (int)pt_family(p, T, R, n, f, sw, force, lane_min), pt_row_capacity(T, n, f, sw));
        } else if (mode == "row") {
            const long R = num(in);
            const int T = (int)num(in), Tg = (int)num(in), n = (int)num(in), flags = (int)num(in), cus = (int)num(in);
            const size_t lds = (size_t)num(in);
            const PtRowPlan pl = pt_row_plan(R, T, Tg, n, flags, cus, lds, switches(in));
            printf("row %d %d %d %d %d %d %ld %d %d %d %d\n", (int)pl.two, (int)pl.win, pl.minw, (int)pl.ho, (int)pl.sl, pl.wpl, pl.grid, pl.rot, pl.xcd_map,
                   (int)pl.cooperative, pl.pipeline);
        } else if (mode == "lad") {
            const int p = (int)num(in), d = (int)num(in), T = (int)num(in);
            const long R = num(in);
            const int n = (int)num(in), cus = (int)num(in);
            const size_t ring = (size_t)num(in);
            const PtLadderPlan pl = pt_ladder_plan(p, d, T, R, n, cus, ring, switches(in));
            printf("lad %d %d %zu %d %d %d %zu\n", (int)pl.fits_pc, pl.nthr_fit, pl.lds_fit, (int)pl.pc, pl.maxt, pl.nthr, pl.lds);
        } else if (mode == "flags") {
            int p = 0, n = 0;
            double max_freq = 0;
            if (!(in >> p >> max_freq >> n) || n < 0) return 2;
            std::vector<double> t((size_t)n);
            for (double& v : t)
                if (!(in >> v)) return 2;
            printf("flags %d\n", series_flags(t.data(), n, p, max_freq));
        } else {
            fprintf(stderr, "plan_main: unknown mode %s\n", mode.c_str());
            return 1;
        }
    }
    return 0;
}
