// carma_post_dev.h -- what the post-processing kernels of carma_post.hip (one series) and carma_mpost.hip (a set) share:
// the spectrum value, the order-preserving keys of the selection, numpy's interpolation, and the host-side launch of the
// grid + row-quantile pair on device-resident inputs.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/carma_mi355.h"

namespace carma {

constexpr int POST_PMAX = CARMA_PMAX;       // AR order <= 7: alpha has <= 8 coefficients, delta <= 7
constexpr int POST_NQ = 8;                  // order statistics per row: two per percentile, four percentiles

// sigma^2 |delta(i w)|^2 / |alpha(i w)|^2, Horner's rule in z = i w:  acc z + c = (c - acc.im w) + i (acc.re w)
// a: nar coefficients highest order first; b: nma coefficients lowest order first; s2 = sigma^2     (carma_pack.py:596-618)
__device__ __forceinline__ double psd_value(int nar, int nma, const double* a, const double* b, double s2, double w)
{
    double are = 0.0, aim = 0.0;
    for (int k = 0; k < nar; k++) {
        const double t = are;
        are = fma(-aim, w, a[k]);
        aim = t * w;
    }
    double mre = 0.0, mim = 0.0;
    for (int k = nma - 1; k >= 0; k--) {
        const double t = mre;
        mre = fma(-mim, w, b[k]);
        mim = t * w;
    }
    return s2 * (mre * mre + mim * mim) / (are * are + aim * aim);
}

// order-preserving image of a double: unsigned comparison of the keys == numerical comparison of the values (-0 < +0)
__device__ __forceinline__ unsigned long long key_of(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(unsigned long long k)
{
    const unsigned long long b = k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
    return __longlong_as_double((long long)b);
}

// numpy's _lerp (np.percentile, method "linear"): a + (b - a) t, from the other end for t >= 0.5
__device__ __forceinline__ double np_lerp(double a, double b, double t)
{
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// np.percentile(x, q) with the default method for a row of ns values: virtual index (ns - 1) q / 100, the order statistics
// either side of it (ranks[0], ranks[1]) and the interpolation weight between them
static inline void percentile_ranks(long ns, double q, int* ranks, double* gamma)
{
    const double vi = (double)(ns - 1) * (q / 100.0);
    double lo = std::floor(vi);
    if (lo > ns - 1) lo = ns - 1;
    const int ilo = (int)lo, ihi = ilo + 1 < ns ? ilo + 1 : (int)(ns - 1);
    ranks[0] = ilo;
    ranks[1] = ihi;
    *gamma = vi - lo;
}

// carma_post.hip: k_psd_grid + k_row_quantiles of ONE series on inputs that are on the device already, enqueued on the null
// stream -- `fc` frequencies at a time through the grid buffer d_grid [fc][ns].  d_ar [nar][ns], d_ma [nma][ns] sample-major.
hipError_t post_grid_band(int nar, int nma, const double* d_ar, const double* d_ma, const double* d_sigma, int ns,
                          const double* d_freq, int nf, int nperc, const int* d_ranks, const double* d_gammas, double* d_grid,
                          int fc, double* d_band /* [nf][nperc] */);
// frequencies the grid buffer holds at a time: at most 2^30 values (8 GiB)
static inline int post_grid_chunk(int nf, long ns) { return (int)std::min<long>(nf, std::max<long>(1, (1L << 30) / ns)); }

}  // namespace carma
