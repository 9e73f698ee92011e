// carma_chaindiag.hip -- chain diagnostics of a whole sampled set in one call (gfx950 only): Goodman's `acor` autocorrelation time
// (MAXLAG 10, WINMULT 5, MINFAC 5), the standard error of the mean that comes with it, and split R-hat over the replicas of a group.
//
// Input x[G][R][L][d], row-major; a chain block is one (g, r): L rows of d adjacent doubles.
//
//   k_chain_diag   one workgroup = one chain block, all d columns together; thread = row lane * dp + column (dp = d padded to a
//                  power of two).  Per level of the estimator: a sweep for the column means, a sweep for the eleven lagged products
//                  of the centred values (rows staged into LDS in tiles of CD_CAP / d - 10 rows with a 10-row halo, centred as they
//                  are stored: the input is never rewritten), the per-column decision, and -- only while a column of the block goes
//                  on -- the halving X'[i] = X[2 i] + X[2 i + 1] of the centred values.  A level that fits the LDS arena lives there
//                  (level 0 too: a short chain is read from HBM once); a longer one is streamed, level 0 from x, later ones from the
//                  block's L / 2 rows of workspace, each halved in place.  Columns stop at different levels: a stopped column is
//                  masked out of the arithmetic and of the stores.  The first sweep of level 0 also gives the sums of the two halves
//                  of the chain and the second their centred sums of squares.
//   k_chain_rhat   one thread per (group, column): split R-hat from those 2 R half means and sums of squares.
//
// Every sum has a fixed order: a thread's rows are its row lane's, partial sums meet in a butterfly over the lanes of a wave and then
// wave by wave.  No floating-point atomics; a block's result depends on L and d alone, not on the launch it is part of.
//
// One deliberate difference from the C original: its recursive call ignores the "series too short" return of the next level and
// silently reports a quarter of the enclosing level's value.  Here a column one of whose levels has fewer than 50 rows before
// tau < 2 is reached comes back with status SHORT and tau = sigma = NaN.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/carma_mi355.h"
#include "carma_chaindiag_plan.h"
#include "carma_host.h"

namespace carma {

constexpr int CD_NW = CD_T / 64;
constexpr int CD_NLAG = CD_MAXLAG + 1;
constexpr int CD_HB = 4;                    // elements per thread of a halving batch
static_assert(CD_NQ * CD_DMAX <= CD_T, "one thread per (quantity, column) in the last step of a reduction");
static_assert(CD_NLAG + 2 <= CD_NQ, "eleven lag sums and the two halves' sums of squares");

struct CdShared {
    double arena[CD_CAP];                   // a tile with its halo, or a whole resident level
    double part[CD_NQ][CD_NW][CD_DMAX];     // per-wave partial sums of a reduction
    double tot[CD_NQ][CD_DMAX];             // ... and its results, per column
    double mean[CD_DMAX];                   // of the current level
    double dl0[CD_DMAX], dl1[CD_DMAX];      // level-0 mean minus the mean of the first / second half
    double c00[CD_DMAX];                    // C[0] of level 0
    double dfin[CD_DMAX], sig[CD_DMAX];     // D and sigma of a column's last level ...
    int last[CD_DMAX];                      // ... and which level that was
    int status[CD_DMAX];
    unsigned active;                        // columns that go on
};

struct CdArgs {
    const double* x;                        // [nb][L][d]
    double* ws;                             // [nb][ws_rows][d]
    long L, ws_rows;
    int d;
    double *tau, *mean, *sigma;             // [nb][d]
    double *hmean, *hm2;                    // [nb][2][d]: mean and centred sum of squares of the first and the last L / 2 rows
    int* status;                            // [nb][d]
};

// Sums of v[0 .. NQ) over the row lanes of every column -> sh.tot[q][column].  Called by all threads of the block.
template <int NQ>
__device__ __forceinline__ void cd_reduce(CdShared& sh, const double (&v)[NQ], int dp, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        double a = v[q];
        for (int off = 32; off >= dp; off >>= 1) a += __shfl_xor(a, off);
        if (lane < dp) sh.part[q][wave][lane] = a;
    }
    __syncthreads();
    if (tid < NQ * dp) {
        const int q = tid / dp, c = tid - q * dp;
        double s = sh.part[q][0][c];
        for (int w = 1; w < CD_NW; w++) s += sh.part[q][w][c];
        sh.tot[q][c] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(CD_T) void k_chain_diag(CdArgs a)
{
    __shared__ CdShared sh;
    const int tid = threadIdx.x, d = a.d, dp = cd_dpad(d);
    const int col = tid & (dp - 1), rl = tid / dp, nrl = CD_T / dp;
    const bool mine = col < d;
    const long blk = blockIdx.x, L = a.L, nh = L / 2;
    const double* xb = a.x + blk * L * d;
    double* wsb = a.ws_rows ? a.ws + blk * a.ws_rows * d : nullptr;
    const int fc = tid % d, fstep = CD_T % d;           // column of a thread's first element of a flat sweep, and its step
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    const double* src = xb;                 // rows of the current level (generic pointer: x, the workspace or the arena)
    bool resident = false;
    if (cd_fits(L, d)) {
        for (int i = tid; i < (int)(L * d); i += CD_T) sh.arena[i] = xb[i];
        src = sh.arena;
        resident = true;
    }
    if (tid < CD_DMAX) {
        sh.status[tid] = CD_OK;
        sh.last[tid] = 0;
        sh.mean[tid] = sh.dl0[tid] = sh.dl1[tid] = sh.c00[tid] = sh.dfin[tid] = sh.sig[tid] = 0.0;
    }
    if (tid == 0) sh.active = (1u << d) - 1u;
    __syncthreads();

    long Lk = L;
    for (int level = 0;; level++) {
        const bool l0 = level == 0;
        // ---- sweep A: column sums (level 0: of the first half, the last half and the middle row; the non-finite count)
        {
            const unsigned act = sh.active;
            double va[4] = {0.0, 0.0, 0.0, 0.0};
            if (mine && ((act >> col) & 1u)) {
                const double* p = src + col;
                if (l0) {
#pragma unroll 4
                    for (long i = rl; i < Lk; i += nrl) {
                        const double v = p[i * d];
                        if (i < nh)
                            va[0] += v;
                        else if (i >= L - nh)
                            va[1] += v;
                        else
                            va[2] += v;
                        if (!__builtin_isfinite(v)) va[3] += 1.0;
                    }
                } else {
#pragma unroll 4
                    for (long i = rl; i < Lk; i += nrl) va[0] += p[i * d];
                }
            }
            cd_reduce<4>(sh, va, dp, tid);
            if (tid < d && ((act >> tid) & 1u)) {
                const double tot = l0 ? (sh.tot[0][tid] + sh.tot[1][tid]) + sh.tot[2][tid] : sh.tot[0][tid];
                const double m = tot / (double)Lk;
                sh.mean[tid] = m;
                if (l0) {
                    const double h0 = sh.tot[0][tid] / (double)nh, h1 = sh.tot[1][tid] / (double)nh;
                    a.mean[blk * d + tid] = m;
                    a.hmean[(blk * 2 + 0) * d + tid] = h0;
                    a.hmean[(blk * 2 + 1) * d + tid] = h1;
                    a.hm2[(blk * 2 + 0) * d + tid] = qnan;
                    a.hm2[(blk * 2 + 1) * d + tid] = qnan;
                    sh.dl0[tid] = m - h0;
                    sh.dl1[tid] = m - h1;
                    if (sh.tot[3][tid] != 0.0) {
                        sh.status[tid] = CD_NONFINITE;
                        atomicAnd(&sh.active, ~(1u << tid));
                    }
                }
            }
            __syncthreads();
        }
        const bool too_short = Lk < CD_MINFAC * CD_MAXLAG;
        if (too_short && !l0) {
            if (tid < d && ((sh.active >> tid) & 1u)) sh.status[tid] = CD_SHORT;
            break;
        }
        // ---- sweep B: lagged products of the centred values (level 0: and the centred squares of the halves, which a chain
        // too short for the estimator still has)
        const unsigned act = sh.active;
        if (act == 0u) break;
        const long imax = too_short ? 0 : Lk - CD_MAXLAG;
        {
            const bool on = mine && ((act >> col) & 1u);
            const double d0 = sh.dl0[col & (CD_DMAX - 1)], d1 = sh.dl1[col & (CD_DMAX - 1)];
            double vb[CD_NLAG + 2];
#pragma unroll
            for (int s = 0; s < CD_NLAG + 2; s++) vb[s] = 0.0;
            const int tr = resident ? (int)Lk : cd_tile_rows(d);
            for (long base = 0; base < Lk; base += tr) {
                const long left = Lk - base;
                const int nrows = (int)(left < tr ? left : tr);
                if (resident) {             // the level is in the arena: centred in place (a copy of ours, not the input)
                    int c = fc;
                    for (int i = tid; i < nrows * d; i += CD_T) {
                        sh.arena[i] -= sh.mean[c];
                        c += fstep;
                        if (c >= d) c -= d;
                    }
                } else {
                    const int nload = (int)(left < tr + CD_MAXLAG ? left : tr + CD_MAXLAG) * d;
                    const double* p = src + base * d;
                    int c = fc;
                    for (int i = tid; i < nload; i += CD_T) {
                        sh.arena[i] = p[i] - sh.mean[c];
                        c += fstep;
                        if (c >= d) c -= d;
                    }
                }
                __syncthreads();
                if (on) {
                    for (int r = rl; r < nrows; r += nrl) {
                        const long i = base + r;
                        const double* t = sh.arena + r * d + col;
                        const double v = t[0];
                        if (l0) {
                            if (i < nh) {
                                const double e = v + d0;
                                vb[CD_NLAG] += e * e;
                            } else if (i >= L - nh) {
                                const double e = v + d1;
                                vb[CD_NLAG + 1] += e * e;
                            }
                        }
                        if (i < imax) {     // i + MAXLAG < Lk: the rows behind it are in the tile or its halo
#pragma unroll
                            for (int s = 0; s < CD_NLAG; s++) vb[s] += v * t[s * d];
                        }
                    }
                }
                __syncthreads();
            }
            cd_reduce<CD_NLAG + 2>(sh, vb, dp, tid);
        }
        // ---- the decision, per column
        if (tid < d && ((act >> tid) & 1u)) {
            bool stop = false;
            if (l0) {
                a.hm2[(blk * 2 + 0) * d + tid] = sh.tot[CD_NLAG][tid];
                a.hm2[(blk * 2 + 1) * d + tid] = sh.tot[CD_NLAG + 1][tid];
            }
            if (too_short) {
                sh.status[tid] = CD_SHORT;
                stop = true;
            } else {
                const double den = (double)imax;
                const double c0 = sh.tot[0][tid] / den;
                double s = 0.0;
                for (int k = 1; k < CD_NLAG; k++) s += sh.tot[k][tid] / den;
                const double D = c0 + 2.0 * s;
                const double sigma = sqrt(D / (double)Lk), tau = D / c0;
                if (l0) {
                    sh.c00[tid] = c0;
                    if (c0 == 0.0) {
                        sh.status[tid] = CD_CONSTANT;
                        stop = true;
                    }
                }
                if (!stop && tau * CD_WINMULT < CD_MAXLAG) {
                    sh.dfin[tid] = D;
                    sh.sig[tid] = sigma;
                    sh.last[tid] = level;
                    stop = true;
                }
            }
            if (stop) atomicAnd(&sh.active, ~(1u << tid));
        }
        __syncthreads();
        const unsigned go = sh.active;
        if (go == 0u) break;
        // ---- halving, for the columns that go on: element e = r d + c of the next level is (X[2 r][c] - m) + (X[2 r + 1][c] - m).
        // It reads elements >= e of this level, so in place every batch of CD_HB CD_T elements is read before it is written, and
        // no later batch reads what an earlier one wrote.
        {
            const long Ln = Lk / 2, nout = Ln * d;
            const bool dst_res = cd_fits(Ln, d);
            double* dst = dst_res ? sh.arena : wsb;
            int c = fc;
            long r = tid / d;
            const int rstep = CD_T / d;
            for (long e0 = 0; e0 < nout; e0 += (long)CD_HB * CD_T) {
                double v[CD_HB];
                bool w[CD_HB];
#pragma unroll
                for (int u = 0; u < CD_HB; u++) {
                    const long e = e0 + (long)u * CD_T + tid;
                    v[u] = 0.0;
                    w[u] = false;
                    if (e < nout) {
                        const double m = resident ? 0.0 : sh.mean[c];
                        const double* p = src + (2 * r) * d + c;
                        v[u] = (p[0] - m) + (p[d] - m);
                        w[u] = (go >> c) & 1u;
                    }
                    c += fstep;
                    r += rstep;
                    if (c >= d) {
                        c -= d;
                        r++;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < CD_HB; u++) {
                    const long e = e0 + (long)u * CD_T + tid;
                    if (w[u]) dst[e] = v[u];
                }
            }
            __syncthreads();
            src = dst;
            resident = dst_res;
            Lk = Ln;
        }
    }
    __syncthreads();
    // ---- unwinding: from a column's last level back to level 0, with each enclosing level's own length
    if (tid < d) {
        const int st = sh.status[tid];
        double tau = qnan, sigma = qnan;
        if (st == CD_OK) {
            double D = sh.dfin[tid];
            sigma = sh.sig[tid];
            for (int k = sh.last[tid] - 1; k >= 0; k--) {
                const double lk = (double)(L >> k);
                D = 0.25 * sigma * sigma * lk;
                sigma = sqrt(D / lk);
            }
            tau = D / sh.c00[tid];
        }
        a.tau[blk * d + tid] = tau;
        a.sigma[blk * d + tid] = sigma;
        a.status[blk * d + tid] = st;
    }
}

// hmean, hm2 [G][R][2][d], status [G][R][d] -> rhat [G][d]
__global__ __launch_bounds__(256) void k_chain_rhat(const double* __restrict__ hmean, const double* __restrict__ hm2,
                                                    const int* __restrict__ status, long G, int R, long L, int d,
                                                    double* __restrict__ rhat)
{
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= G * d) return;
    const long g = o / d;
    const int c = (int)(o - g * d);
    const long n = L / 2;
    double out = __longlong_as_double(0x7ff8000000000000ll);
    bool ok = n >= 2;
    for (int r = 0; r < R && ok; r++) ok = status[(g * R + r) * d + c] != CD_NONFINITE;
    if (ok) {
        const double* hm = hmean + g * R * 2 * d + c;
        const double* h2 = hm2 + g * R * 2 * d + c;
        const int nhalf = 2 * R;
        double sw = 0.0, sm = 0.0;
        for (int k = 0; k < nhalf; k++) {
            sw += h2[(long)k * d] / (double)(n - 1);
            sm += hm[(long)k * d];
        }
        const double W = sw / nhalf, mm = sm / nhalf;
        double sb = 0.0;
        for (int k = 0; k < nhalf; k++) {
            const double e = hm[(long)k * d] - mm;
            sb += e * e;
        }
        const double B = (double)n * (sb / (double)(nhalf - 1));
        if (W != 0.0) out = sqrt((((double)(n - 1) / (double)n) * W + B / (double)n) / W);
    }
    rhat[o] = out;
}

}  // namespace carma

using namespace carma;

static double g_cd_kernel_ms = -1.0;        // device time of the kernels of the last call that succeeded (measurements)

extern "C" {

int carma_chain_diag_dmax(void) { return CD_DMAX; }

double carma_chain_diag_kernel_ms(void) { return g_cd_kernel_ms; }

int carma_chain_diag(const double* x, long ngroups, int nreplicas, long nsamples, int d, double* tau, double* mean, double* sigma,
                     int* status, double* rhat, int device)
{
    if (!x || !tau || !mean || !sigma || !status || ngroups < 1 || nreplicas < 1 || nsamples < 1 || d < 1 || d > CD_DMAX) {
        set_error("carma_chain_diag: bad argument (x, tau, mean, sigma, status not null; ngroups, nreplicas, nsamples >= 1; 1 <= d <= %d)",
                  CD_DMAX);
        return CARMA_EINVAL;
    }
    ChainDiagPlan pl;
    if (!cd_plan(ngroups, nreplicas, nsamples, d, &pl)) {
        set_error("carma_chain_diag: ngroups x nreplicas (at most 2^31 - 1 chain blocks) or the whole array is too large for one call");
        return CARMA_EINVAL;
    }
    int rc = select_device(device);
    if (rc != CARMA_OK) return rc;
    DevMem dev;
    std::vector<unsigned char> out(pl.out_bytes());
    hipError_t e = dev.alloc(pl.bytes);
    unsigned char* base = dev.as<unsigned char>();
    if (e == hipSuccess) e = hipMemcpy(base + pl.o_x, x, sizeof(double) * (size_t)pl.nb * (size_t)nsamples * d, hipMemcpyHostToDevice);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (e == hipSuccess) e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, nullptr);
    if (e == hipSuccess) {
        CdArgs a;
        a.x = reinterpret_cast<const double*>(base + pl.o_x);
        a.ws = reinterpret_cast<double*>(base + pl.o_ws);
        a.L = nsamples;
        a.ws_rows = pl.ws_rows;
        a.d = d;
        a.tau = reinterpret_cast<double*>(base + pl.o_tau);
        a.mean = reinterpret_cast<double*>(base + pl.o_mean);
        a.sigma = reinterpret_cast<double*>(base + pl.o_sigma);
        a.hmean = reinterpret_cast<double*>(base + pl.o_hmean);
        a.hm2 = reinterpret_cast<double*>(base + pl.o_hm2);
        a.status = reinterpret_cast<int*>(base + pl.o_status);
        hipLaunchKernelGGL(k_chain_diag, dim3((unsigned)pl.nb), dim3(CD_T), 0, nullptr, a);
        e = hipGetLastError();
        if (e == hipSuccess && rhat) {
            const long nrh = ngroups * d;
            hipLaunchKernelGGL(k_chain_rhat, dim3((unsigned)((nrh + 255) / 256)), dim3(256), 0, nullptr, a.hmean, a.hm2, a.status,
                               ngroups, nreplicas, nsamples, d, reinterpret_cast<double*>(base + pl.o_rhat));
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipEventRecord(ev1, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out.data(), base + pl.o_out, pl.out_bytes(), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    float ms = -1.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (e != hipSuccess) return hip_fail(e, "carma_chain_diag");
    g_cd_kernel_ms = ms;
    const size_t nbd = (size_t)pl.nb * d;
    std::memcpy(tau, out.data() + (pl.o_tau - pl.o_out), sizeof(double) * nbd);
    std::memcpy(mean, out.data() + (pl.o_mean - pl.o_out), sizeof(double) * nbd);
    std::memcpy(sigma, out.data() + (pl.o_sigma - pl.o_out), sizeof(double) * nbd);
    std::memcpy(status, out.data() + (pl.o_status - pl.o_out), sizeof(int) * nbd);
    if (rhat) std::memcpy(rhat, out.data() + (pl.o_rhat - pl.o_out), sizeof(double) * (size_t)ngroups * d);
    return CARMA_OK;
}

}  // extern "C"
