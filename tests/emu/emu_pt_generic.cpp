// emu_pt_generic.cpp -- the REFERENCE LADDER of the sampler tests: ram_propose / ram_finish / exchange_sweep of carma_pt_core.h
// on the host, for chains of ANY dimension d (those routines take a run-time d: they are the project's own definition of an
// iteration) with the log-density supplied by the caller.  A group of one lane; R ladders of T chains, chain = ladder * T +
// temperature keys the Philox streams, as the lane sampler's kernels key them.  TEST HARNESS ONLY.
//
//   emu_pt_generic(dens, user, d, T, R, temps, maxiter, iter0, niter, thin, seed0, seed1, theta, lp, chol, samples, sample_lp,
//                  nacc, nswap)
// runs iterations iter0 ... iter0 + niter - 1 (the chains adapt while the iteration index is below maxiter).  theta [R T][d],
// lp [R T], chol [R T][d d] (upper triangular, row-major) are the chains' state, in and out; nacc / nswap [R T] are added to
// (nswap[ladder T + i]: swaps between temperatures i and i - 1).  thin > 0: after every thin-th iteration of THIS call the
// coldest chain of every ladder is saved, samples [R][niter / thin][d], sample_lp [R][niter / thin].
// dens(thn [nc][d], nc, out [nc], user) -> 0 or an error code, which ends the run and is returned.
#include <cstdint>
#include <cstring>
#include <vector>

#include "grp_emu.h"
#include "../../carma_pack_amd/csrc/carma_pt_core.h"

using namespace carma;

typedef int (*dens_cb)(const double* thn, int nc, double* out, void* user);

extern "C" int emu_pt_generic(dens_cb dens, void* user, int d, int T, int R, const double* temps, int maxiter,
                              unsigned long long iter0, long niter, int thin, unsigned seed0, unsigned seed1, double* theta, double* lp,
                              double* chol, double* samples, double* sample_lp, unsigned* nacc, unsigned* nswap)
{
    if (d < 1 || T < 1 || R < 1 || niter < 0 || thin < 0) return -22;
    const int nc = R * T;
    const long cap = thin > 0 ? niter / thin : 0;
    EmuShared sh;
    sh.bar.n = 1;
    const Grp<1> g{&sh, 0};
    // per chain: th and thn are rows of two [nc][d] arrays (the exchange sweep strides over th, dens reads thn), z, v, R apart
    std::vector<double> thn((size_t)nc * d), z((size_t)nc * d), v((size_t)nc * d), ll(nc), z2(nc);
    auto scratch = [&](int c) {
        ChainScratch cs;
        cs.th = theta + (size_t)c * d;
        cs.thn = thn.data() + (size_t)c * d;
        cs.z = z.data() + (size_t)c * d;
        cs.v = v.data() + (size_t)c * d;
        cs.R = chol + (size_t)c * d * d;
        return cs;
    };
    for (long it = 0; it < niter; it++) {
        const uint64_t iter = iter0 + (uint64_t)it;
        for (int c = 0; c < nc; c++) z2[c] = ram_propose<1>(g, scratch(c), d, iter, RngKey{seed0, seed1, (uint32_t)c});
        const int rc = dens(thn.data(), nc, ll.data(), user);
        if (rc != 0) return rc;
        for (int c = 0; c < nc; c++)
            if (ram_finish<1>(g, scratch(c), d, temps[c % T], iter, maxiter, RngKey{seed0, seed1, (uint32_t)c}, ll[c], z2[c], &lp[c]))
                nacc[c]++;
        for (int l = 0; l < R; l++) {
            if (T > 1)
                exchange_sweep(T, d, d, theta + (size_t)l * T * d, lp + (size_t)l * T, temps, RngKey{seed0, seed1, 0u}, (uint32_t)(l * T),
                               iter, nswap + (size_t)l * T);
            if (thin > 0 && ((it + 1) % thin) == 0) {
                const long s = (it + 1) / thin - 1;
                std::memcpy(samples + ((size_t)l * cap + s) * d, theta + (size_t)l * T * d, sizeof(double) * d);
                sample_lp[(size_t)l * cap + s] = lp[(size_t)l * T];
            }
        }
    }
    return 0;
}
