// devprim.hip -- TEST HARNESS ONLY: thin kernels around the device building blocks of carma_pack_amd/csrc (carma_math.h,
// grp_device.h, carma_row_asm.h, carma_rng.h, and of the windowed pipeline carma_pipew.h: pipew_merge, WinAsm<P>::init / ::chunk,
// recip, rsqrt_pos), one primitive call per lane, arguments and results in plain arrays.
// tests/devprim_ref.py builds it into tests/devprim/libdevprim.so and loads it with ctypes; the product never loads it.
//
// Every launcher: allocate, copy in, launch, synchronise, copy out, free; returns 0 or the HIP error code.  Launches are
// full waves only (n must be a multiple of the block size, 64 or 256): the cross-lane primitives are not meant for
// partially active waves.
#include "grp_device.h"
#include "carma_math.h"
#include "carma_rng.h"
#include "carma_core.h"
#include "carma_pipew.h"

#include <cstdint>
#include <vector>

using namespace carma;

namespace {

struct Bufs {
    std::vector<void*> p;
    hipError_t err = hipSuccess;
    template <class T>
    T* in(const T* host, size_t count)
    {
        T* d = out<T>(count);
        if (err == hipSuccess && count) err = hipMemcpy(d, host, sizeof(T) * count, hipMemcpyHostToDevice);
        return d;
    }
    template <class T>
    T* out(size_t count)
    {
        void* d = nullptr;
        if (err == hipSuccess) {
            err = hipMalloc(&d, sizeof(T) * (count ? count : 1));
            if (err == hipSuccess) p.push_back(d);
        }
        return (T*)d;
    }
    template <class T>
    void back(T* host, const T* dev, size_t count)
    {
        if (err == hipSuccess && count) err = hipMemcpy(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost);
    }
    void ran()
    {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    int done()
    {
        for (void* d : p) {
            hipError_t e = hipFree(d);
            if (err == hipSuccess) err = e;
        }
        p.clear();
        return (int)err;
    }
};

bool full_waves(int n, int threads) { return n > 0 && (threads == 64 || threads == 256) && n % threads == 0; }

// ------------------------------------------------------------------------------------------------------------ math
enum { F_EXP_NEG, F_EXP_NEG_TAB, F_SINCOS_CW, F_CEXP, F_CEXP_TAB, F_CEXP_EXACT, F_CEXP_TAB_EXACT, F_RECIP, F_RSQRT_POS, F_RCP_RAW,
       F_RSQ_RAW, F_COUNT };

template <int FN>
__global__ __launch_bounds__(256) void k_math(int n, const double* __restrict__ a, const double* __restrict__ b,
                                              const double* __restrict__ dt, const double* __restrict__ dt_lo,
                                              double* __restrict__ o0, double* __restrict__ o1)
{
    __shared__ double tab[MATH_TAB_N];
    math_tab_fill(tab);
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r0 = 0.0, r1 = 0.0;
    if constexpr (FN == F_EXP_NEG) r0 = exp_neg(a[i]);
    if constexpr (FN == F_EXP_NEG_TAB) r0 = exp_neg_tab(a[i], tab);
    if constexpr (FN == F_SINCOS_CW) sincos_cw(a[i], &r0, &r1);
    if constexpr (FN == F_CEXP) cexp_step<false>(a[i], b[i], dt[i], &r0, &r1);
    if constexpr (FN == F_CEXP_TAB) cexp_step_tab<false>(a[i], b[i], dt[i], &r0, &r1, tab);
    if constexpr (FN == F_CEXP_EXACT) cexp_step<true>(a[i], b[i], dt[i], &r0, &r1, dt_lo[i]);
    if constexpr (FN == F_CEXP_TAB_EXACT) cexp_step_tab<true>(a[i], b[i], dt[i], &r0, &r1, tab);
    if constexpr (FN == F_RECIP) r0 = recip(a[i]);
    if constexpr (FN == F_RSQRT_POS) r0 = rsqrt_pos(a[i]);
    if constexpr (FN == F_RCP_RAW) r0 = __builtin_amdgcn_rcp(a[i]);
    if constexpr (FN == F_RSQ_RAW) r0 = __builtin_amdgcn_rsq(a[i]);
    o0[i] = r0;
    o1[i] = r1;
}

// ------------------------------------------------------------------------------------------------------ lane groups
// per lane: GRP_IN doubles in, one int in, the source lane j of the run-time broadcasts, a flag for wave_all
constexpr int GRP_IN = 4;
// per lane out (64-bit words): see devprim_ref.py GRP_*
constexpr int GO_SUM = 0, GO_MAX = 1, GO_PARTNER = 2, GO_BC_C = 3, GO_BC_CI = 19, GO_BC_U = 35, GO_BC_IU = 51, GO_BCAST = 67,
              GO_BCAST_I = 68, GO_PEEK = 69, GO_PEEKK2 = 133, GO_PEEK2 = 149, GO_WAVE_ALL = 181, GRP_OUT = 182;

__device__ __forceinline__ unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ unsigned long long bits(int v) { return (unsigned long long)(unsigned)v; }

template <int G, int J>
__device__ __forceinline__ void bcast_c_all(double v, int iv, unsigned long long* o)
{
    if constexpr (J < G) {
        o[GO_BC_C + J] = bits(Grp<G>::template bcast_c<J>(v));
        o[GO_BC_CI + J] = bits(Grp<G>::template bcast_c<J>(iv));
        bcast_c_all<G, J + 1>(v, iv, o);
    }
}

template <int G>
__global__ __launch_bounds__(256) void k_grp(int n, const double* __restrict__ in, const int* __restrict__ iin,
                                             const int* __restrict__ jsrc, const int* __restrict__ flag,
                                             unsigned long long* __restrict__ out)
{
    __shared__ double4 xch[256];
    __shared__ double2 xch2[256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int wave = threadIdx.x >> 6;
    Grp<G> g;
    g.xch = xch + 64 * wave;
    g.lane64 = threadIdx.x & 63;
    g.xch2 = xch2 + 64 * wave;
    const double v = in[(size_t)i * GRP_IN], v1 = in[(size_t)i * GRP_IN + 1], v2 = in[(size_t)i * GRP_IN + 2],
                 v3 = in[(size_t)i * GRP_IN + 3];
    const int iv = iin[i], j = jsrc[i];
    unsigned long long* o = out + (size_t)i * GRP_OUT;
    o[GO_SUM] = bits(Grp<G>::sum(v));
    o[GO_MAX] = bits(Grp<G>::max(v));
    o[GO_PARTNER] = bits(Grp<G>::partner(v));
    bcast_c_all<G, 0>(v, iv, o);
#pragma unroll
    for (int k = 0; k < G; k++) {
        o[GO_BC_U + k] = bits(g.bcast_u(v, k));
        o[GO_BC_IU + k] = bits(g.bcast_iu(iv, k));
    }
    o[GO_BCAST] = bits(g.bcast(v, j));
    o[GO_BCAST_I] = bits(g.bcast_i(iv, j));
    g.publish(v, v1, v2, v3);
    for (int k = 0; k < G; k++) {
        const double4 q = g.peek(k);
        o[GO_PEEK + 4 * k] = bits(q.x);
        o[GO_PEEK + 4 * k + 1] = bits(q.y);
        o[GO_PEEK + 4 * k + 2] = bits(q.z);
        o[GO_PEEK + 4 * k + 3] = bits(q.w);
    }
    g.done_reading();
    g.publishk(v1);
    for (int k = 0; k < G / 2; k++) {
        double a, b;
        g.peekk2(k, a, b);
        o[GO_PEEKK2 + 2 * k] = bits(a);
        o[GO_PEEKK2 + 2 * k + 1] = bits(b);
    }
    g.done_reading();
    g.publish2(v2, v3);
    for (int k = 0; k < G; k++) {
        const Cx c = g.peek2(k);
        o[GO_PEEK2 + 2 * k] = bits(c.re);
        o[GO_PEEK2 + 2 * k + 1] = bits(c.im);
    }
    g.done_reading();
    o[GO_WAVE_ALL] = Grp<G>::wave_all(flag[i] != 0) ? 1ull : 0ull;
}

// ------------------------------------------------------------------------------------------------------- row blocks
// per lane in: c, s, D[7], ht, ct, scale, s0, S[7], k, nt, mu, z;  out: mm[7], w, var, k, S'[7], innov
constexpr int RI_C = 0, RI_S = 1, RI_D = 2, RI_HT = 9, RI_CT = 10, RI_SCALE = 11, RI_S0 = 12, RI_SS = 13, RI_K = 20, RI_NT = 21,
              RI_MU = 22, RI_Z = 23, ROW_IN = 24;
constexpr int RO_MM = 0, RO_W = 7, RO_VAR = 8, RO_K = 9, RO_SS = 10, RO_INNOV = 17, ROW_OUT = 18;

// e and y are kernel arguments: wave-uniform by construction (the blocks take them in SGPRs)
template <int P>
__global__ __launch_bounds__(256) void k_row(int n, const double* __restrict__ in, double e, double y, double* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* x = in + (size_t)i * ROW_IN;
    double* o = out + (size_t)i * ROW_OUT;
    const double one = 1.0;
    double D[P], S[P], mm[P];
#pragma unroll
    for (int j = 0; j < P; j++) {
        D[j] = x[RI_D + j];
        S[j] = x[RI_SS + j];
    }
    RowAsm<P>::colmix(mm, x[RI_C], x[RI_S], D);
    double w, var, k;
    RowAsm<P>::lazy_front(w, var, k, x[RI_HT], x[RI_CT], e, x[RI_SCALE], x[RI_S0], one, S);
    double innov;
    RowAsm<P>::innov_t2(innov, y, x[RI_MU], x[RI_Z], x[RI_HT], one);
    RowAsm<P>::gain_nt(S, x[RI_K], x[RI_NT]);
#pragma unroll
    for (int j = 0; j < P; j++) {
        o[RO_MM + j] = mm[j];
        o[RO_SS + j] = S[j];
    }
    o[RO_W] = w;
    o[RO_VAR] = var;
    o[RO_K] = k;
    o[RO_INNOV] = innov;
}

// ------------------------------------------------------------------------------------------- two-sided merge, window blocks
// One wave per block.  The merge: per lane in kf[P], nu (carma_pipew.h: the virtual lanes ND + j of rows 0 / 2 carry column j of Da
// and -a_j, those of rows 1 / 3 column j of Db and -beta_j); out {acc.total(), the row pair's sum as pipew_recur forms it}.
template <int P>
__global__ __launch_bounds__(64) void k_merge(int n, const double* __restrict__ in, double* __restrict__ out)
{
    __shared__ double2 ring[PipeWGeom<P>::ENTRIES];
    const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
    if (i >= n) return;                                       // (never: full waves only)
    const double* x = in + (size_t)i * (P + 1);
    double kf[P];
#pragma unroll
    for (int r = 0; r < P; r++) kf[r] = x[r];
    const double nu = x[P];
    LogLikAcc acc;
    acc.init();
    pipew_merge<P>(lane, kf, nu, ring, acc);
    const double tot = acc.total();
    double ll = Grp<16>::sum(tot);
    ll += __shfl_xor(ll, 16, 64);
    out[(size_t)i * 2] = tot;
    out[(size_t)i * 2 + 1] = ll;
}

// WinAsm<P>::init -- per lane in: kn[P], nun, kk[P], nuF, hn[P];  out: kn[P], nun
template <int P>
__global__ __launch_bounds__(64) void k_win_init(int n, const double* __restrict__ in, double* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* x = in + (size_t)i * (3 * P + 2);
    double kn[P], kk[P], hn[P];
#pragma unroll
    for (int r = 0; r < P; r++) {
        kn[r] = x[r];
        kk[r] = x[P + 1 + r];
        hn[r] = x[2 * P + 2 + r];
    }
    double nun = x[P];
    const double nuF = x[2 * P + 1];
    WinAsm<P>::init(kn, nun, kk, nuF, hn);
#pragma unroll
    for (int r = 0; r < P; r++) out[(size_t)i * (P + 1) + r] = kn[r];
    out[(size_t)i * (P + 1) + P] = nun;
}

// WinAsm<P>::chunk -- per lane in: kk[P], hh[P], m, nu (mA = mB = m, nuA = nuB = nu, as the start of a chunk leaves them);
// out: kk[P], mA, mB, nuA, nuB.  MASKED: the call sits under `if (row active)` (rows: bits of a kernel argument), outputs and a
// marker are stored by the lanes that are active BEHIND the call -- the block narrows EXEC and has to hand the caller's mask back.
template <int P, bool MASKED>
__global__ __launch_bounds__(64) void k_win_chunk(int n, int rows, const double* __restrict__ in, double* __restrict__ out,
                                                  int* __restrict__ marker)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double* x = in + (size_t)i * (2 * P + 2);
    double* o = out + (size_t)i * (P + 4);
    double kk[P], hh[P];
#pragma unroll
    for (int r = 0; r < P; r++) {
        kk[r] = x[r];
        hh[r] = x[P + r];
    }
    double mA = x[2 * P], mB = mA, nuA = x[2 * P + 1], nuB = nuA;
    if (!MASKED || ((rows >> (threadIdx.x >> 4)) & 1)) {
        __builtin_amdgcn_sched_barrier(0);
        WinAsm<P>::chunk(kk, hh, mA, mB, nuA, nuB);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < P; r++) o[r] = kk[r];
        o[P] = mA;
        o[P + 1] = mB;
        o[P + 2] = nuA;
        o[P + 3] = nuB;
        marker[i] = 1;
    }
}

// -------------------------------------------------------------------------------------------------------------- RNG
// words: [n][6] c0 c1 c2 c3 k0 k1 -> out [n][4], u [n] = u01(out0, out1)
__global__ __launch_bounds__(256) void k_philox(int n, const uint32_t* __restrict__ words, uint32_t* __restrict__ out,
                                                double* __restrict__ u)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = words + (size_t)i * 6;
    const Philox4 x = philox4x32_10(w[0], w[1], w[2], w[3], w[4], w[5]);
    for (int k = 0; k < 4; k++) out[(size_t)i * 4 + k] = x.v[k];
    u[i] = u01(x.v[0], x.v[1]);
}

// key: [n][5] k0 k1 chain purpose idx;  out [n][3]: rng_uniform(purpose, idx), rng_normal(idx), rng_student_t8(idx)
__global__ __launch_bounds__(256) void k_rng(int n, const uint32_t* __restrict__ key, const unsigned long long* __restrict__ iter,
                                             double* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = key + (size_t)i * 5;
    const RngKey rk{w[0], w[1], w[2]};
    out[(size_t)i * 3] = rng_uniform(rk, iter[i], w[3], w[4]);
    out[(size_t)i * 3 + 1] = rng_normal(rk, iter[i], w[4]);
    out[(size_t)i * 3 + 2] = rng_student_t8(rk, iter[i], w[4]);
}

}  // namespace

extern "C" {

int devprim_device_count()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int devprim_math(int fn, int n, int threads, const double* a, const double* b, const double* dt, const double* dt_lo, double* o0,
                 double* o1)
{
    if (!full_waves(n, threads) || fn < 0 || fn >= F_COUNT) return (int)hipErrorInvalidValue;
    Bufs B;
    const double *da = B.in(a, n), *db = B.in(b, n), *dd = B.in(dt, n), *dl = B.in(dt_lo, n);
    double *d0 = B.out<double>(n), *d1 = B.out<double>(n);
    if (B.err == hipSuccess) {
        const dim3 grid(n / threads), block(threads);
        switch (fn) {
#define DEVPRIM_MATH_CASE(F) \
    case F: hipLaunchKernelGGL(k_math<F>, grid, block, 0, nullptr, n, da, db, dd, dl, d0, d1); break;
            DEVPRIM_MATH_CASE(F_EXP_NEG)
            DEVPRIM_MATH_CASE(F_EXP_NEG_TAB)
            DEVPRIM_MATH_CASE(F_SINCOS_CW)
            DEVPRIM_MATH_CASE(F_CEXP)
            DEVPRIM_MATH_CASE(F_CEXP_TAB)
            DEVPRIM_MATH_CASE(F_CEXP_EXACT)
            DEVPRIM_MATH_CASE(F_CEXP_TAB_EXACT)
            DEVPRIM_MATH_CASE(F_RECIP)
            DEVPRIM_MATH_CASE(F_RSQRT_POS)
            DEVPRIM_MATH_CASE(F_RCP_RAW)
            DEVPRIM_MATH_CASE(F_RSQ_RAW)
#undef DEVPRIM_MATH_CASE
        }
        B.ran();
    }
    B.back(o0, d0, n);
    B.back(o1, d1, n);
    return B.done();
}

int devprim_grp(int G, int n, int threads, const double* in, const int* iin, const int* jsrc, const int* flag,
                unsigned long long* out)
{
    if (!full_waves(n, threads) || !(G == 2 || G == 4 || G == 8 || G == 16)) return (int)hipErrorInvalidValue;
    Bufs B;
    const double* di = B.in(in, (size_t)n * GRP_IN);
    const int *dv = B.in(iin, n), *dj = B.in(jsrc, n), *df = B.in(flag, n);
    unsigned long long* d_o = B.out<unsigned long long>((size_t)n * GRP_OUT);
    if (B.err == hipSuccess) B.err = hipMemset(d_o, 0, sizeof(unsigned long long) * (size_t)n * GRP_OUT);
    if (B.err == hipSuccess) {
        const dim3 grid(n / threads), block(threads);
        if (G == 2) hipLaunchKernelGGL(k_grp<2>, grid, block, 0, nullptr, n, di, dv, dj, df, d_o);
        if (G == 4) hipLaunchKernelGGL(k_grp<4>, grid, block, 0, nullptr, n, di, dv, dj, df, d_o);
        if (G == 8) hipLaunchKernelGGL(k_grp<8>, grid, block, 0, nullptr, n, di, dv, dj, df, d_o);
        if (G == 16) hipLaunchKernelGGL(k_grp<16>, grid, block, 0, nullptr, n, di, dv, dj, df, d_o);
        B.ran();
    }
    B.back(out, d_o, (size_t)n * GRP_OUT);
    return B.done();
}

int devprim_row(int P, int n, int threads, const double* in, double e, double y, double* out)
{
    if (!full_waves(n, threads) || P < 2 || P > 7) return (int)hipErrorInvalidValue;
    Bufs B;
    const double* di = B.in(in, (size_t)n * ROW_IN);
    double* d_o = B.out<double>((size_t)n * ROW_OUT);
    if (B.err == hipSuccess) {
        const dim3 grid(n / threads), block(threads);
        switch (P) {
            case 2: hipLaunchKernelGGL(k_row<2>, grid, block, 0, nullptr, n, di, e, y, d_o); break;
            case 3: hipLaunchKernelGGL(k_row<3>, grid, block, 0, nullptr, n, di, e, y, d_o); break;
            case 4: hipLaunchKernelGGL(k_row<4>, grid, block, 0, nullptr, n, di, e, y, d_o); break;
            case 5: hipLaunchKernelGGL(k_row<5>, grid, block, 0, nullptr, n, di, e, y, d_o); break;
            case 6: hipLaunchKernelGGL(k_row<6>, grid, block, 0, nullptr, n, di, e, y, d_o); break;
            case 7: hipLaunchKernelGGL(k_row<7>, grid, block, 0, nullptr, n, di, e, y, d_o); break;
        }
        B.ran();
    }
    B.back(out, d_o, (size_t)n * ROW_OUT);
    return B.done();
}

#define DEVPRIM_FOR_P(CALL) \
    switch (P) {            \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
        case 5: CALL(5); break; \
        case 6: CALL(6); break; \
        case 7: CALL(7); break; \
    }

// in [nblocks * 64][P + 1], out [nblocks * 64][2]
int devprim_merge(int P, int nblocks, const double* in, double* out)
{
    if (nblocks <= 0 || P < 2 || P > 7) return (int)hipErrorInvalidValue;
    const int n = nblocks * 64;
    Bufs B;
    const double* di = B.in(in, (size_t)n * (P + 1));
    double* d_o = B.out<double>((size_t)n * 2);
    if (B.err == hipSuccess) {
#define DEVPRIM_CALL(Q) hipLaunchKernelGGL(k_merge<Q>, dim3(nblocks), dim3(64), 0, nullptr, n, di, d_o)
        DEVPRIM_FOR_P(DEVPRIM_CALL)
#undef DEVPRIM_CALL
        B.ran();
    }
    B.back(out, d_o, (size_t)n * 2);
    return B.done();
}

// in [nblocks * 64][3 P + 2], out [nblocks * 64][P + 1]
int devprim_win_init(int P, int nblocks, const double* in, double* out)
{
    if (nblocks <= 0 || P < 2 || P > 7) return (int)hipErrorInvalidValue;
    const int n = nblocks * 64;
    Bufs B;
    const double* di = B.in(in, (size_t)n * (3 * P + 2));
    double* d_o = B.out<double>((size_t)n * (P + 1));
    if (B.err == hipSuccess) {
#define DEVPRIM_CALL(Q) hipLaunchKernelGGL(k_win_init<Q>, dim3(nblocks), dim3(64), 0, nullptr, n, di, d_o)
        DEVPRIM_FOR_P(DEVPRIM_CALL)
#undef DEVPRIM_CALL
        B.ran();
    }
    B.back(out, d_o, (size_t)n * (P + 1));
    return B.done();
}

namespace {
// in [n][2 P + 2]; out [n][P + 4] and marker [n] keep what the caller put there in the lanes that store nothing
int win_chunk(int P, int nblocks, bool masked, int rows, const double* in, double* out, int* marker)
{
    if (nblocks <= 0 || P < 2 || P > 7) return (int)hipErrorInvalidValue;
    const int n = nblocks * 64;
    Bufs B;
    const double* di = B.in(in, (size_t)n * (2 * P + 2));
    double* d_o = B.in(out, (size_t)n * (P + 4));
    int* dm = B.in(marker, n);
    if (B.err == hipSuccess) {
#define DEVPRIM_CALL(Q)                                                                                          \
    if (masked)                                                                                                  \
        hipLaunchKernelGGL((k_win_chunk<Q, true>), dim3(nblocks), dim3(64), 0, nullptr, n, rows, di, d_o, dm);   \
    else                                                                                                         \
        hipLaunchKernelGGL((k_win_chunk<Q, false>), dim3(nblocks), dim3(64), 0, nullptr, n, rows, di, d_o, dm)
        DEVPRIM_FOR_P(DEVPRIM_CALL)
#undef DEVPRIM_CALL
        B.ran();
    }
    B.back(out, d_o, (size_t)n * (P + 4));
    B.back(marker, dm, n);
    return B.done();
}
}  // namespace

int devprim_win_chunk(int P, int nblocks, const double* in, double* out, int* marker)
{
    return win_chunk(P, nblocks, false, 0xf, in, out, marker);
}

// rows: bit q set = row q of every wave is active at the call
int devprim_win_chunk_masked(int P, int nblocks, int rows, const double* in, double* out, int* marker)
{
    return win_chunk(P, nblocks, true, rows & 0xf, in, out, marker);
}

int devprim_philox(int n, int threads, const uint32_t* words, uint32_t* out, double* u)
{
    if (!full_waves(n, threads)) return (int)hipErrorInvalidValue;
    Bufs B;
    const uint32_t* dw = B.in(words, (size_t)n * 6);
    uint32_t* d_o = B.out<uint32_t>((size_t)n * 4);
    double* du = B.out<double>(n);
    if (B.err == hipSuccess) {
        hipLaunchKernelGGL(k_philox, dim3(n / threads), dim3(threads), 0, nullptr, n, dw, d_o, du);
        B.ran();
    }
    B.back(out, d_o, (size_t)n * 4);
    B.back(u, du, n);
    return B.done();
}

int devprim_rng(int n, int threads, const uint32_t* key, const unsigned long long* iter, double* out)
{
    if (!full_waves(n, threads)) return (int)hipErrorInvalidValue;
    Bufs B;
    const uint32_t* dk = B.in(key, (size_t)n * 5);
    const unsigned long long* dit = B.in(iter, n);
    double* d_o = B.out<double>((size_t)n * 3);
    if (B.err == hipSuccess) {
        hipLaunchKernelGGL(k_rng, dim3(n / threads), dim3(threads), 0, nullptr, n, dk, dit, d_o);
        B.ran();
    }
    B.back(out, d_o, (size_t)n * 3);
    return B.done();
}

}  // extern "C"
