// carma_model_pack.h -- a fitted model as the KalmanFilterp-type kernels read it: the order of the AR roots, the row of the
// batched entry points and the block of the single-model ones.  Plain C++, host only.  The entry points keep their own argument
// checks, loops and error texts; nothing here sets one.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/carma_mi355.h"

namespace carma {

// AR roots as the kernels expect them: complex-conjugate pairs adjacent (negative imaginary part first), real roots
// after them -- the order CARp::ARRoots emits (src/carpack.cpp:137-172).  The result of the filter does not depend on
// the order of the roots, so roots handed over in another order (carma_pack.py's get_ar_roots puts a real root wherever
// its centroid is zero) are re-ordered here; a set that is not closed under conjugation is not a real-valued process
// and is rejected (CARMA_EINVAL).  out = p (re, im) pairs.
inline int normalize_roots(int p, const double* om, double* out)
{
    std::vector<int> used(p, 0);
    int k = 0;
    for (int i = 0; i < p; i++) {
        if (used[i] || om[2 * i + 1] == 0.0) continue;
        const double re = om[2 * i], im = om[2 * i + 1], tol = 1e-12 * std::hypot(re, im);
        int mate = -1;
        for (int j = i + 1; j < p && mate < 0; j++)
            if (!used[j] && std::fabs(om[2 * j] - re) <= tol && std::fabs(om[2 * j + 1] + im) <= tol) mate = j;
        if (mate < 0) return CARMA_EINVAL;
        used[i] = used[mate] = 1;
        out[2 * k] = out[2 * k + 2] = re;
        out[2 * k + 1] = -std::fabs(im);
        out[2 * k + 3] = std::fabs(im);
        k += 2;
    }
    for (int i = 0; i < p; i++) {
        if (used[i]) continue;
        out[2 * k] = om[2 * i];
        out[2 * k + 1] = 0.0;
        k++;
    }
    return CARMA_OK;
}

// One row of a model batch, 3 p + 2 wide: [2 p roots, normalised][p MA coefficients: ma[0 .. nma), zero padded
// (kfilter.hpp:318-320)][sigsqr][mu].  nma <= p.  CARMA_EINVAL when the roots are not closed under conjugation.
inline int pack_model_row(int p, const double* om_re_im, const double* ma, int nma, double sigsqr, double mu, double* row)
{
    if (normalize_roots(p, om_re_im, row) != CARMA_OK) return CARMA_EINVAL;
    std::copy(ma, ma + nma, row + 2 * p);
    std::fill(row + 2 * p + nma, row + 3 * p, 0.0);
    row[3 * p] = sigsqr;
    row[3 * p + 1] = mu;
    return CARMA_OK;
}

// The block of the single-model kernels: [2 CARMA_PMAX: the 2 p roots, normalised, then zeros][CARMA_PMAX: the first
// min(p, nma) MA coefficients, then zeros]
inline int pack_model_single(int p, const double* om_re_im, const double* ma, int nma, double* par)
{
    if (normalize_roots(p, om_re_im, par) != CARMA_OK) return CARMA_EINVAL;
    std::fill(par + 2 * p, par + 2 * CARMA_PMAX, 0.0);
    const int m = std::min(p, nma);
    std::copy(ma, ma + m, par + 2 * CARMA_PMAX);
    std::fill(par + 2 * CARMA_PMAX + m, par + 3 * CARMA_PMAX, 0.0);
    return CARMA_OK;
}

}  // namespace carma
