// carma_mpost.hip -- the power-spectrum band of EVERY series of a sampled set in one call (gfx950 only).
//
// carma_psd_band (carma_post.hip) serves one series with 5e4 .. 3e6 samples: it writes the [nf][ns] grid to HBM and reads it
// back with one 1024-thread workgroup per frequency.  A set run has the opposite shape -- a thousand series with a few hundred
// samples each -- and there a row of the grid fits the LDS of a CU many times over:
//
//   k_mpsd_fused   one workgroup = one series x a tile of MPSD_FT frequencies.  The spectrum values of R frequencies at a time
//                  (R rows of npad keys, npad = the series' sample count rounded up to a power of two, R npad <= the launch's
//                  LDS) are formed straight into LDS as their order-preserving 64-bit keys, every row is sorted there by a
//                  bitonic network (all R rows in the same steps), and the 2 nperc order statistics are picked from the sorted
//                  row: nperc doubles per (series, frequency) are all that reaches HBM.
// Series with more than MPSD_FUSED_MAX samples take the grid path of carma_post.hip inside the same host call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/carma_mi355.h"
#include "carma_host.h"
#include "carma_post_dev.h"

namespace carma {

constexpr int MPSD_T = 512;                 // threads of k_mpsd_fused: 8 waves, two workgroups give each SIMD 4
constexpr int MPSD_FT = 32;                 // frequencies per workgroup
constexpr int MPSD_NPAD_MIN = 64;           // a row is padded to at least one wave of keys
// The keys of a row stay in LDS: 160 KiB per CU, two workgroups resident -> 80 KiB = 10240 keys per workgroup; the sorting network
// wants a power of two, so 8192 keys (64 KiB) it is.
constexpr int MPSD_FUSED_MAX = 8192;
constexpr unsigned long long MPSD_PAD_KEY = ~0ull;   // above every key of a number and of +inf (it is the image of a NaN pattern)

struct MpsdSeries {                         // one fused series as the kernel sees it
    long start;                             // first sample: the coefficient blocks of the series begin at start * nar, start * nma
    int ns, npad;
    int series;                             // index in the caller's order (frequency grid, band rows)
    int ranks[POST_NQ];
    double gammas[POST_NQ / 2];
};

// ar: per series [nar][ns] (sample-major within the series, at start * nar), ma likewise; sigma [N]; freq [nseries][nf];
// band [nseries][nf][nperc].  Dynamic LDS: `cap` keys, cap >= npad of every series of the launch.
__global__ __launch_bounds__(MPSD_T) void k_mpsd_fused(int nar, int nma, const double* __restrict__ ar, const double* __restrict__ ma,
                                                        const double* __restrict__ sigma, const MpsdSeries* __restrict__ items,
                                                        int ntiles, const double* __restrict__ freq, int nf, int nperc, int cap,
                                                        double* __restrict__ band)
{
    extern __shared__ unsigned long long keys[];
    const MpsdSeries* it = items + blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles, tid = threadIdx.x;
    const int ns = it->ns, npad = it->npad;
    const long start = it->start;
    const double* a_s = ar + start * nar;
    const double* b_s = ma + start * nma;
    const double* fr = freq + (long)it->series * nf;
    double* out = band + (long)it->series * nf * nperc;
    const int f_begin = tile * MPSD_FT, f_end = min(nf, f_begin + MPSD_FT);
    const int rmax = min(cap / npad, MPSD_FT);                // rows (frequencies) in LDS at a time
    // npad <= MPSD_T: a thread meets the same sample in every row -- its coefficients are loaded once, into registers
    const bool resident = npad <= MPSD_T;
    double a[POST_PMAX + 1], b[POST_PMAX + 1], s2 = 0.0;
    const int smp0 = tid & (npad - 1);
    if (resident && smp0 < ns) {
        for (int k = 0; k < nar; k++) a[k] = a_s[(long)k * ns + smp0];
        for (int k = 0; k < nma; k++) b[k] = b_s[(long)k * ns + smp0];
        const double sg = sigma[start + smp0];
        s2 = sg * sg;
    }
    for (int f0 = f_begin; f0 < f_end; f0 += rmax) {
        const int R = min(rmax, f_end - f0), total = R * npad;
        for (int i = tid; i < total; i += MPSD_T) {
            const int r = i / npad, smp = i & (npad - 1);
            unsigned long long key = MPSD_PAD_KEY;
            if (smp < ns) {
                if (!resident) {
                    for (int k = 0; k < nar; k++) a[k] = a_s[(long)k * ns + smp];
                    for (int k = 0; k < nma; k++) b[k] = b_s[(long)k * ns + smp];
                    const double sg = sigma[start + smp];
                    s2 = sg * sg;
                }
                const double w = 2.0 * M_PI * fr[f0 + r];
                key = key_of(psd_value(nar, nma, a, b, s2, w));
            }
            keys[i] = key;
        }
        __syncthreads();
        // bitonic network on every row at once: compare-exchange c of a step pairs i (bit j clear) with i | j, ascending where
        // the row-local index has bit k clear
        const int half = total >> 1;
        for (int k = 2; k <= npad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int c = tid; c < half; c += MPSD_T) {
                    const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1)), l = i | j;
                    const bool up = ((i & (npad - 1)) & k) == 0;
                    const unsigned long long x = keys[i], y = keys[l];
                    if ((x > y) == up) {
                        keys[i] = y;
                        keys[l] = x;
                    }
                }
                __syncthreads();
            }
        }
        // a NaN sorts below every number (sign bit set) or above +inf: the ends of the sorted row tell whether there is one
        for (int o = tid; o < R * nperc; o += MPSD_T) {
            const int r = o / nperc, j = o - r * nperc;
            const unsigned long long* row = keys + r * npad;
            const double lo = value_of(row[0]), hi = value_of(row[ns - 1]);
            double v = __longlong_as_double(0x7ff8000000000000ll);   // np.percentile: a NaN anywhere in the row makes every percentile NaN
            if (lo == lo && hi == hi) v = np_lerp(value_of(row[it->ranks[2 * j]]), value_of(row[it->ranks[2 * j + 1]]), it->gammas[j]);
            out[(long)(f0 + r) * nperc + j] = v;
        }
        __syncthreads();
    }
}

static inline size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace carma

using namespace carma;

extern "C" {

int carma_mpsd_fused_max(void) { return MPSD_FUSED_MAX; }

int carma_mpsd_freq_tile(void) { return MPSD_FT; }

int carma_mpsd_band(int nar, int nma, const double* ar_coefs, const double* ma_coefs, const double* sigma, const long* sample_start,
                    int nseries, const double* freq, int nf, const double* percentiles, int nperc, double* band, int device)
{
    if (nar < 2 || nar > CARMA_PMAX + 1 || nma < 1 || nma > CARMA_PMAX || !ar_coefs || !ma_coefs || !sigma || !sample_start ||
        !freq || !percentiles || !band || nseries < 1 || nf < 1 || nperc < 1 || 2 * nperc > POST_NQ) {
        set_error("carma_mpsd_band: bad argument (2 <= nar <= %d, 1 <= nma <= %d, nseries >= 1, nf >= 1, 1 ... %d percentiles)",
                  CARMA_PMAX + 1, CARMA_PMAX, POST_NQ / 2);
        return CARMA_EINVAL;
    }
    if (sample_start[0] != 0) {
        set_error("carma_mpsd_band: sample_start[0] must be 0");
        return CARMA_EINVAL;
    }
    for (int s = 0; s < nseries; s++)
        if (sample_start[s + 1] <= sample_start[s] || sample_start[s + 1] - sample_start[s] > 0x7fffffffL) {
            set_error("carma_mpsd_band: sample_start must increase strictly (series %d), by less than 2^31", s);
            return CARMA_EINVAL;
        }
    for (int j = 0; j < nperc; j++)
        if (!(percentiles[j] >= 0.0 && percentiles[j] <= 100.0)) {
            set_error("carma_mpsd_band: percentiles must lie in [0, 100]");   // numpy: ValueError
            return CARMA_EINVAL;
        }
    if ((double)nseries * nf * nperc >= 9.0e15 || (double)nseries * (nf + MPSD_FT) > 2.0e9 * MPSD_FT) {
        set_error("carma_mpsd_band: nseries x nf is too large for one call");
        return CARMA_EINVAL;
    }
    int rc = select_device(device);
    if (rc != CARMA_OK) return rc;
    const long N = sample_start[nseries];
    // one host block, one device block, one copy: [ar, per series sample-major][ma likewise][sigma][freq][fused items]
    // [ranks and gammas of the series on the grid path]
    std::vector<int> big;
    int nfused = 0, cap = 0;
    long grid_vals = 0;
    for (int s = 0; s < nseries; s++) {
        const long ns = sample_start[s + 1] - sample_start[s];
        if (ns <= MPSD_FUSED_MAX) {
            nfused++;
        } else {
            big.push_back(s);
            grid_vals = std::max(grid_vals, (long)post_grid_chunk(nf, ns) * ns);
        }
    }
    const size_t o_ar = 0, o_ma = o_ar + round16(sizeof(double) * N * nar), o_sg = o_ma + round16(sizeof(double) * N * nma),
                 o_fr = o_sg + round16(sizeof(double) * N), o_it = o_fr + round16(sizeof(double) * (size_t)nseries * nf),
                 o_gm = o_it + round16(sizeof(MpsdSeries) * (size_t)nfused),
                 o_rk = o_gm + round16(sizeof(double) * (POST_NQ / 2) * big.size()),
                 bytes = o_rk + round16(sizeof(int) * POST_NQ * big.size());
    std::vector<unsigned char> host(bytes, 0);
    double* h_ar = reinterpret_cast<double*>(host.data() + o_ar);
    double* h_ma = reinterpret_cast<double*>(host.data() + o_ma);
    MpsdSeries* h_it = reinterpret_cast<MpsdSeries*>(host.data() + o_it);
    double* h_gm = reinterpret_cast<double*>(host.data() + o_gm);
    int* h_rk = reinterpret_cast<int*>(host.data() + o_rk);
    std::memcpy(host.data() + o_sg, sigma, sizeof(double) * N);
    std::memcpy(host.data() + o_fr, freq, sizeof(double) * (size_t)nseries * nf);
    int fi = 0, bi = 0;
    for (int s = 0; s < nseries; s++) {
        const long st = sample_start[s], ns = sample_start[s + 1] - st;
        double* at = h_ar + st * nar;
        double* mt = h_ma + st * nma;
        for (long i = 0; i < ns; i++) {
            for (int k = 0; k < nar; k++) at[(size_t)k * ns + i] = ar_coefs[(size_t)(st + i) * nar + k];
            for (int k = 0; k < nma; k++) mt[(size_t)k * ns + i] = ma_coefs[(size_t)(st + i) * nma + k];
        }
        int ranks[POST_NQ] = {0};
        double gam[POST_NQ / 2] = {0.0};
        for (int j = 0; j < nperc; j++) percentile_ranks(ns, percentiles[j], ranks + 2 * j, gam + j);
        if (ns <= MPSD_FUSED_MAX) {
            MpsdSeries& m = h_it[fi++];
            m.start = st;
            m.ns = (int)ns;
            m.npad = MPSD_NPAD_MIN;
            while (m.npad < ns) m.npad <<= 1;
            m.series = s;
            std::memcpy(m.ranks, ranks, sizeof(ranks));
            std::memcpy(m.gammas, gam, sizeof(gam));
            cap = std::max(cap, m.npad);
        } else {
            std::memcpy(h_rk + (size_t)bi * POST_NQ, ranks, sizeof(ranks));
            std::memcpy(h_gm + (size_t)bi * (POST_NQ / 2), gam, sizeof(gam));
            bi++;
        }
    }
    // LDS of the launch: room for a whole frequency tile of the widest row, at most the fused limit
    cap = std::min(MPSD_FUSED_MAX, cap * MPSD_FT);
    DevMem d_in, d_band, d_grid;
    const size_t nband = (size_t)nseries * nf * nperc;
    hipError_t e = d_in.alloc(bytes);
    if (e == hipSuccess) e = d_band.alloc(sizeof(double) * nband);
    if (e == hipSuccess && !big.empty()) e = d_grid.alloc(sizeof(double) * (size_t)grid_vals);
    if (e == hipSuccess) e = hipMemcpy(d_in.as<void>(), host.data(), bytes, hipMemcpyHostToDevice);
    const unsigned char* base = d_in.as<const unsigned char>();
    const double* g_ar = reinterpret_cast<const double*>(base + o_ar);
    const double* g_ma = reinterpret_cast<const double*>(base + o_ma);
    const double* g_sg = reinterpret_cast<const double*>(base + o_sg);
    const double* g_fr = reinterpret_cast<const double*>(base + o_fr);
    double* g_band = d_band.as<double>();
    if (e == hipSuccess && nfused > 0) {
        const int ntiles = (nf + MPSD_FT - 1) / MPSD_FT;
        hipLaunchKernelGGL(k_mpsd_fused, dim3((unsigned)((long)nfused * ntiles)), dim3(MPSD_T), sizeof(unsigned long long) * cap,
                           nullptr, nar, nma, g_ar, g_ma, g_sg, reinterpret_cast<const MpsdSeries*>(base + o_it), ntiles, g_fr, nf,
                           nperc, cap, g_band);
        e = hipGetLastError();
    }
    for (size_t k = 0; k < big.size() && e == hipSuccess; k++) {
        const int s = big[k];
        const long st = sample_start[s], ns = sample_start[s + 1] - st;
        e = post_grid_band(nar, nma, g_ar + st * nar, g_ma + st * nma, g_sg + st, (int)ns, g_fr + (size_t)s * nf, nf, nperc,
                           reinterpret_cast<const int*>(base + o_rk) + k * POST_NQ,
                           reinterpret_cast<const double*>(base + o_gm) + k * (POST_NQ / 2), d_grid.as<double>(),
                           post_grid_chunk(nf, ns), g_band + (size_t)s * nf * nperc);
    }
    if (e == hipSuccess) e = hipMemcpy(band, g_band, sizeof(double) * nband, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "carma_mpsd_band");
    return CARMA_OK;
}

}  // extern "C"
