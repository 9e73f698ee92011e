// emu_smooth.cpp -- builds carma_pack_amd/csrc/carma_smooth.h for the host with the lane emulator.
// TEST HARNESS ONLY (see grp_emu.h): the two passes of the one-pass smoother exactly as the gfx950 kernel compiles them,
// one OS thread per lane, the grid from carma_smooth_plan.h.
#include <vector>
#include "grp_emu.h"
#include "../../carma_pack_amd/csrc/carma_smooth.h"
#include "../../carma_pack_amd/csrc/carma_smooth_plan.h"

using namespace carma;

template <int P>
struct GroupOf {
    static constexpr int value = P <= 2 ? 2 : (P <= 4 ? 4 : 8);
};

// om = P (re, im) pairs, conjugate pairs adjacent; ma = P coefficients, zero padded
template <int P>
static void smooth_one(const double* om, const double* ma, double sigsqr, double mu, const double4* series,
                       const SmoothGrid& sg, double* mean, double* var, int* sing)
{
    constexpr int G = GroupOf<P>::value;
    std::vector<double4> rec((size_t)sg.ng * G), grp((size_t)sg.ng);
    run_group<G>([&](const Grp<G>& g) {
        Model<P> m;
        model_from_roots<P, G>(g, om, ma, sigsqr, m);
        FilterConsts<P> fc;
        filter_reset<P, G>(g, m, fc);
        smooth_forward<P, G>(g, m, fc, series, sg.grid.data(), sg.src.data(), sg.ng, mu, rec.data() + g.lane(), G, grp.data(), 1);
        g.sync();
        smooth_backward<P, G>(g, fc, sg.src.data(), sg.ng, mu, rec.data() + g.lane(), G, grp.data(), 1, mean, var);
        if (g.lane() == 0) *sing = fc.sing;
    });
}

extern "C" int emu_smooth_carma(int p, const double* om, const double* ma, double sigsqr, double mu, const double* series,
                                int n, const double* tout, int M, double* mean, double* var)
{
    const double4* s4 = reinterpret_cast<const double4*>(series);
    std::vector<double> t(n);
    for (int j = 0; j < n; j++) t[j] = s4[j].w;
    const SmoothGrid sg = smooth_merge(t.data(), n, tout, M);
    int sing = 0;
    switch (p) {
        case 2: smooth_one<2>(om, ma, sigsqr, mu, s4, sg, mean, var, &sing); break;
        case 3: smooth_one<3>(om, ma, sigsqr, mu, s4, sg, mean, var, &sing); break;
        case 4: smooth_one<4>(om, ma, sigsqr, mu, s4, sg, mean, var, &sing); break;
        case 5: smooth_one<5>(om, ma, sigsqr, mu, s4, sg, mean, var, &sing); break;
        case 6: smooth_one<6>(om, ma, sigsqr, mu, s4, sg, mean, var, &sing); break;
        case 7: smooth_one<7>(om, ma, sigsqr, mu, s4, sg, mean, var, &sing); break;
        default: return -1;
    }
    return sing;
}

extern "C" void emu_smooth_car1(double sigsqr, double omega, double mu, const double* series, int n, const double* tout, int M,
                                double* mean, double* var)
{
    const double4* s4 = reinterpret_cast<const double4*>(series);
    std::vector<double> t(n);
    for (int j = 0; j < n; j++) t[j] = s4[j].w;
    const SmoothGrid sg = smooth_merge(t.data(), n, tout, M);
    std::vector<double> sc((size_t)5 * sg.ng);
    smooth_car1(sigsqr, omega, mu, s4, sg.grid.data(), sg.src.data(), sg.ng, sc.data(), 1, sg.ng, mean, var);
}
