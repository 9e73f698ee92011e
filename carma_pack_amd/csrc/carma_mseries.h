// carma_mseries.h -- what the multi-series translation units share (carma_mseries.hip: context and log-density;
// carma_mitems.hip: Filter(), Predict and the smoother of (series, model) items; carma_mpt.hip: the sampler): the context, the
// sampler state (MptState, carma_pt_state.h), the item packer and the small host helpers of the item calls.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/carma_mi355.h"
#include "carma_host.h"
#include "carma_mseries_plan.h"
#include "carma_pt_sched.h"

namespace carma {

// Multi-series context: the series of a set packed one after another in HBM, each as carma_ctx_create packs one
struct Mctx {
    std::unique_ptr<MptState> mpt;    // sampler state of carma_mpt_create, if any
    int device = 0;
    int p = 0, q = 0, d = 0, S = 0;
    std::vector<long> hoff;           // [S + 1] start of series s in t / y / yerr (after sort/dedup)
    std::vector<double> t, y, yerr;   // all series, sorted and deduplicated, concatenated
    std::vector<long> off;            // [S] first record of series s in d_rec (a multiple of 2 records: 64-byte aligned)
    std::vector<int> n;               // [S]
    std::vector<Prior> pr;            // [S]
    std::vector<char> repdt;          // [S] SERIES_REPEATED_DT of each series
    DevMem d_rec, d_off, d_n, d_pr;   // records of all series; [S] each: off, n, pr
    const double4* rec() const { return d_rec.as<const double4>(); }
    const long* offs() const { return d_off.as<const long>(); }
    const int* ns() const { return d_n.as<const int>(); }
    const Prior* prs() const { return d_pr.as<const Prior>(); }
    WaveBatch wb;                     // per-call buffers and launch plan of carma_mlogdensity_batch (carma_devbuf.h)
    hipStream_t stream = nullptr;
    // carma_mkfilter / carma_mpredict / carma_msmooth: parameters and times (doubles), plan tables (ints, longs), tiles, results,
    // flags; grown by DevMem::need
    DevMem k_par, k_int, k_long, k_tile, k_res, k_sing;
};

// The items of carma_mkfilter / carma_mpredict / carma_msmooth -> par [M][3 p + 2] (p = 1: [M][3]: sigsqr, omega, mu) in the
// caller's order, as the kernels read them.  Host only; an argument error names its item.
inline int pack_items(const Mctx* c, const char* who, const int* series, int M, const double* sigsqr, const double* om,
                      const double* ma, int nma, const double* mu, std::vector<double>& par)
{
    const int p = c->p;
    if (M < 1 || !series || !sigsqr || !om || (p > 1 && (!ma || nma < 1 || nma > p))) {
        set_error("%s: bad argument (M >= 1, non-null arrays, 1 <= nma <= p; got M=%d nma=%d p=%d)", who, M, nma, p);
        return CARMA_EINVAL;
    }
    const int PW = p == 1 ? 3 : 3 * p + 2;
    par.assign((size_t)M * PW, 0.0);
    for (int i = 0; i < M; i++) {
        if (series[i] < 0 || series[i] >= c->S) {
            set_error("%s: item %d: series index %d out of range (nseries = %d)", who, i, series[i], c->S);
            return CARMA_EINVAL;
        }
        if (p == 1) {
            double* pb = par.data() + (size_t)i * PW;
            if (om[2 * (size_t)i + 1] != 0.0) {
                set_error("%s: item %d: the root of a CAR(1) model must be real", who, i);
                return CARMA_EINVAL;
            }
            pb[0] = sigsqr[i];
            pb[1] = -om[2 * (size_t)i];
            pb[2] = mu ? mu[i] : 0.0;
            continue;
        }
        if (pack_model_row(p, om + (size_t)i * 2 * p, ma + (size_t)i * nma, nma, sigsqr[i], mu ? mu[i] : 0.0,
                           par.data() + (size_t)i * PW) != CARMA_OK) {
            set_error("%s: item %d: the AR roots must be real or come in complex-conjugate pairs", who, i);
            return CARMA_EINVAL;
        }
    }
    return CARMA_OK;
}

// check_toff with the error worded for `who`
inline int toff_ok(const char* who, const long* toff, int M)
{
    const long i = check_toff(toff, M);
    if (i == TOFF_OK) return CARMA_OK;
    if (i == TOFF_NEGATIVE)
        set_error("%s: toff[0] = %ld is negative", who, toff[0]);
    else
        set_error("%s: item %ld: toff must be non-decreasing (toff[%ld]=%ld > toff[%ld]=%ld)", who, i, i, toff[i], i + 1, toff[i + 1]);
    return CARMA_EINVAL;
}

template <class T>
inline hipError_t upload(DevMem& b, const std::vector<T>& v, hipStream_t st)
{
    hipError_t e = b.need(sizeof(T) * v.size());
    if (e == hipSuccess) e = hipMemcpyAsync(b.as<void>(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st);
    return e;
}

// The end of an item call, whatever e its enqueueing gave: wait for the stream -- also after a failure, since enqueued copies read
// and write the caller's frame -- and report.
inline int finish_items(const char* who, hipError_t e, hipStream_t st)
{
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    return e == hipSuccess ? CARMA_OK : hip_fail(e, who);
}

}  // namespace carma
