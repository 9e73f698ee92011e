// carma_capi.hip -- C ABI of libcarma_mi355.so (see include/carma_mi355.h for the contract and
// the reference interface each entry point replaces).  Host side only: argument checking, the
// series preparation of KalmanFilter::init, HBM residency, launches.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "../../include/carma_mi355.h"
#include "carma_host.h"

// ---- device allocations (carma_devbuf.h) -----------------------------------------------------------------------
#include <map>
#include <mutex>
namespace {
struct GuardAlloc {
    hipMemGenericAllocationHandle_t handle;
    void* base;
    size_t reserved, mapped;
};
std::mutex g_guard_mu;
std::map<void*, GuardAlloc> g_guard;      // user pointer -> mapping
bool guard_mode()
{
    static const bool on = [] {
        const char* e = getenv("CARMA_DEBUG_GUARD");
        return e && e[0] == '1';
    }();
    return on;
}
}  // namespace
hipError_t carma_dev_malloc(void** p, size_t n)
{
    if (!guard_mode()) return ::hipMalloc(p, n);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
    if (e != hipSuccess) return e;
    if (gran == 0) gran = 2u << 20;
    const size_t need = n ? n : 1;
    GuardAlloc a{};
    a.mapped = (need + gran - 1) / gran * gran;
    a.reserved = a.mapped + gran;                             // one granule of address space behind the buffer stays unmapped
    e = hipMemAddressReserve(&a.base, a.reserved, gran, nullptr, 0);
    if (e != hipSuccess) return e;
    e = hipMemCreate(&a.handle, a.mapped, &prop, 0);
    if (e == hipSuccess) e = hipMemMap(a.base, a.mapped, 0, a.handle, 0);
    if (e == hipSuccess) {
        hipMemAccessDesc acc = {};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(a.base, a.mapped, &acc, 1);
    }
    if (e != hipSuccess) {
        (void)hipMemAddressFree(a.base, a.reserved);
        return e;
    }
    // the buffer ENDS where the mapping ends (16-byte alignment: up to 15 bytes of slack behind odd sizes)
    const size_t user = (need + 15) / 16 * 16;
    *p = static_cast<char*>(a.base) + (a.mapped - user);
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guard[*p] = a;
    return hipSuccess;
}
hipError_t carma_pinned_malloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
hipError_t carma_pinned_free(void* p) { return hipHostFree(p); }
hipError_t carma_dev_free(void* p)
{
    if (!p) return hipSuccess;
    if (!guard_mode()) return ::hipFree(p);
    GuardAlloc a{};
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        auto it = g_guard.find(p);
        if (it == g_guard.end()) return hipErrorInvalidValue;
        a = it->second;
        g_guard.erase(it);
    }
    (void)hipDeviceSynchronize();                             // (hipFree's implicit synchronisation)
    hipError_t e = hipMemUnmap(a.base, a.mapped);
    if (e == hipSuccess) e = hipMemRelease(a.handle);
    // (the address range stays reserved for the life of the process: an address is never handed out twice, so a pointer
    // used after its buffer was freed faults as well)
    return e;
}

namespace carma {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what)
{
    set_error("%s: %s", what, hipGetErrorString(e));
    (void)hipGetLastError();
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) ? CARMA_ENODEV
           : (e == hipErrorOutOfMemory)                                                             ? CARMA_ENOMEM
                                                                                                    : CARMA_EHIP;
}

// series records {dt_k, y_k, yerr_k^2, t_k}
std::vector<double> pack_series(const std::vector<double>& t, const std::vector<double>& y, const std::vector<double>& e)
{
    const size_t n = t.size(), nt = n + P3L_PAD_RECORDS;
    std::vector<double> s(6 * nt);
    for (size_t k = 0; k < n; k++) {
        s[4 * k + 0] = k ? t[k] - t[k - 1] : 0.0;
        s[4 * k + 1] = y[k];
        s[4 * k + 2] = e[k] * e[k];
        s[4 * k + 3] = t[k];
    }
    for (size_t k = n; k < n + P3L_PAD_RECORDS; k++) {        // neutral pad records (carma_types.h, p3l_pad)
        s[4 * k + 0] = 0.0;
        s[4 * k + 1] = n ? y[n - 1] : 0.0;
        s[4 * k + 2] = 1.0;
        s[4 * k + 3] = n ? t[n - 1] : 0.0;
    }
    // behind the records: yerr^2 and y once more as plain arrays -- the recursion waves of the pipeline fetch sixteen
    // of them per chunk with scalar loads, and contiguous doubles come in two wide loads instead of sixteen
    for (size_t k = 0; k < nt; k++) {
        s[4 * nt + k] = s[4 * k + 2];
        s[5 * nt + k] = s[4 * k + 1];
    }
    return s;
}

int select_device(int device)
{
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device visible (this library has no CPU fallback)");
        return CARMA_ENODEV;
    }
    if (device < 0 || device >= cnt) {
        set_error("device %d out of range (have %d)", device, cnt);
        return CARMA_EINVAL;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return CARMA_OK;
}

int Ctx::ensure_staging(int B)
{
    if (B <= cap) return CARMA_OK;
    d_theta.release();
    d_out.release();
    h_stage.release();
    cap = 0;
    int newcap = std::max(B, 1024);
    hipError_t e = d_theta.alloc((size_t)newcap * d);
    if (e != hipSuccess) return hip_fail(e, "device staging (theta)");
    e = d_out.alloc((size_t)newcap);
    if (e != hipSuccess) return hip_fail(e, "device staging (out)");
    // pinned, so that both copies are real asynchronous DMA transfers ordered on the stream (a copy from pageable memory
    // is staged by the runtime and synchronises)
    e = h_stage.alloc((size_t)newcap * (d + 1));
    if (e != hipSuccess) return hip_fail(e, "pinned staging");
    cap = newcap;
    return CARMA_OK;
}

}  // namespace carma

using namespace carma;

extern "C" {

const char* carma_version(void) { return "carma_mi355 0.1 (gfx950)"; }
const char* carma_last_error(void) { return g_err; }

int carma_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return cnt;
}

carma_ctx* carma_ctx_create(const double* time, const double* y, const double* yerr, int n, int p, int q,
                            double max_stdev, int device)
{
    if (!time || !y || !yerr || n < 2) {
        set_error("carma_ctx_create: need n >= 2 and non-null arrays");
        return nullptr;
    }
    if (p < 1 || p > CARMA_PMAX || q < 0 || (p == 1 && q != 0) || (p > 1 && q >= p)) {
        // BOOST_ASSERT_MSG(q < p, ...) src/include/carpack.hpp:377
        set_error("carma_ctx_create: need 1 <= p <= %d and q < p (got p=%d q=%d)", CARMA_PMAX, p, q);
        return nullptr;
    }
    if (select_device(device) != CARMA_OK) return nullptr;
    Ctx* c = new Ctx();
    c->device = device;
    c->p = p;
    c->q = q;
    c->d = (p == 1) ? 4 : 3 + p + q;
    c->t.assign(time, time + n);
    c->y.assign(y, y + n);
    c->yerr.assign(yerr, yerr + n);
    sort_dedup(c->t, c->y, c->yerr);
    c->n = (int)c->t.size();
    if (c->n < 2) {
        set_error("carma_ctx_create: fewer than 2 distinct times");
        delete c;
        return nullptr;
    }
    c->pr.measerr_dof = 50.0;   // src/include/carpack.hpp:63
    carma_ctx_set_prior(reinterpret_cast<carma_ctx*>(c), max_stdev);
    std::vector<double> s = pack_series(c->t, c->y, c->yerr);
    c->sflags = series_flags(c->t.data(), c->n, p, c->pr.max_freq);
    hipError_t e = c->d_series.alloc(s.size());
    if (e == hipSuccess) e = hipMemcpy(c->d_series, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        hip_fail(e, "carma_ctx_create");
        carma_ctx_destroy(reinterpret_cast<carma_ctx*>(c));
        return nullptr;
    }
    return reinterpret_cast<carma_ctx*>(c);
}

void carma_ctx_destroy(carma_ctx* h)
{
    if (!h) return;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                                 // (its members release their buffers, the sampler state among them)
}

int carma_ctx_n(const carma_ctx* h) { return h ? reinterpret_cast<const Ctx*>(h)->n : CARMA_EINVAL; }
int carma_ctx_dim(const carma_ctx* h) { return h ? reinterpret_cast<const Ctx*>(h)->d : CARMA_EINVAL; }

int carma_ctx_get_data(const carma_ctx* h, double* time, double* y, double* yerr)
{
    if (!h) return CARMA_EINVAL;
    const Ctx* c = reinterpret_cast<const Ctx*>(h);
    if (time) std::memcpy(time, c->t.data(), sizeof(double) * c->n);
    if (y) std::memcpy(y, c->y.data(), sizeof(double) * c->n);
    if (yerr) std::memcpy(yerr, c->yerr.data(), sizeof(double) * c->n);
    return CARMA_OK;
}

int carma_ctx_get_prior(const carma_ctx* h, double* out3)
{
    if (!h || !out3) return CARMA_EINVAL;
    prior_out3(reinterpret_cast<const Ctx*>(h)->pr, out3);
    return CARMA_OK;
}

int carma_ctx_set_prior(carma_ctx* h, double max_stdev)
{
    if (!h) return CARMA_EINVAL;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    set_prior_bounds(c->pr, c->t.data(), c->n, max_stdev);
    return CARMA_OK;
}

int carma_logdensity_batch_dev(carma_ctx* h, const double* d_theta, int B, int ignore_prior, double* d_out, void* stream)
{
    if (!h || !d_theta || !d_out || B < 0) {
        set_error("carma_logdensity_batch_dev: bad argument");
        return CARMA_EINVAL;
    }
    if (B == 0) return CARMA_OK;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e;
    if (c->p == 1)
        e = launch_logdens_car1(d_theta, B, c->rec(), c->n, c->pr, d_out, st);
    else
        e = launch_logdens_carma(c->p, d_theta, B, c->d, c->q, c->rec(), c->n, c->pr, ignore_prior, d_out, st, c->series_flags());
    if (e != hipSuccess) return hip_fail(e, "launch logdensity");
    return CARMA_OK;
}

int carma_logdensity_batch(carma_ctx* h, const double* theta, int B, int ignore_prior, double* out)
{
    if (!h || !theta || !out || B < 0) {
        set_error("carma_logdensity_batch: bad argument");
        return CARMA_EINVAL;
    }
    if (B == 0) return CARMA_OK;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    int rc = c->ensure_staging(B);
    if (rc != CARMA_OK) return rc;
    // host -> pinned -> device, launch, device -> pinned: three stream-ordered operations and ONE synchronisation
    double* h_th = c->h_stage;
    double* h_out = c->h_stage + (size_t)c->cap * c->d;
    std::memcpy(h_th, theta, sizeof(double) * (size_t)B * c->d);
    if (B <= 4096) {
        // small batches: the kernel reads its parameter vectors from, and writes its results to, the pinned buffer
        // itself (device-visible host memory) -- a read of d doubles per evaluation over the link at the start of the
        // kernel instead of two copy operations around it
        rc = carma_logdensity_batch_dev(h, h_th, B, ignore_prior, h_out, c->stream);
        if (rc != CARMA_OK) return rc;
        e = hipStreamSynchronize(c->stream);              // (polling hipStreamQuery instead: 2 us slower, measured)
        if (e != hipSuccess) return hip_fail(e, "logdensity (pinned)");
        std::memcpy(out, h_out, sizeof(double) * (size_t)B);
        return CARMA_OK;
    }
    e = hipMemcpyAsync(c->d_theta, h_th, sizeof(double) * (size_t)B * c->d, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e, "H2D theta");
    rc = carma_logdensity_batch_dev(h, c->d_theta, B, ignore_prior, c->d_out, c->stream);
    if (rc != CARMA_OK) return rc;
    e = hipMemcpyAsync(h_out, c->d_out, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "D2H logdensity");
    std::memcpy(out, h_out, sizeof(double) * (size_t)B);
    return CARMA_OK;
}

int carma_logdensity_kernel_name(const carma_ctx* h, int B, char* buf, int len)
{
    if (!h || !buf || len < 1 || B < 1) return CARMA_EINVAL;
    const Ctx* c = reinterpret_cast<const Ctx*>(h);
    return logdens_kernel_name(c->p, B, c->n, buf, len, c->series_flags()) > 0 ? CARMA_OK : CARMA_EINVAL;
}

int carma_tune_set(const char* name, long value) { return tune_set(name, value) == 0 ? CARMA_OK : CARMA_EINVAL; }

int carma_normalize_roots(int p, const double* omega_re_im, double* out)
{
    if (p < 1 || p > CARMA_PMAX || !omega_re_im || !out) return CARMA_EINVAL;
    return normalize_roots(p, omega_re_im, out);
}

double carma_logprior(const carma_ctx* h, const double* theta)
{
    if (!h || !theta) return std::numeric_limits<double>::quiet_NaN();
    const Ctx* c = reinterpret_cast<const Ctx*>(h);
    // src/include/carpack.hpp:118-126
    const double s = theta[1];
    return -0.5 * c->pr.measerr_dof / s - (1.0 + c->pr.measerr_dof / 2.0) * std::log(s);
}

}  // extern "C"

namespace carma {

// KalmanFilter1 / KalmanFilterp object (kfilter.hpp:211-334): the sorted / deduplicated series and the model, resident
// in HBM for the life of the handle (the free functions below build one per call).
struct Kf {
    int device = 0, p = 0, n = 0;
    double sigsqr = 0.0, car1_omega = 0.0;
    DevMem d_series, d_par, d_io, d_sing;                    // d_io: exactly what the largest call so far asked for
    hipStream_t stream = nullptr;
    int ensure_io(size_t nd)
    {
        if (sizeof(double) * nd <= d_io.capacity()) return CARMA_OK;
        const hipError_t e = d_io.alloc(sizeof(double) * nd);
        return e == hipSuccess ? CARMA_OK : hip_fail(e, "carma_kf: hipMalloc");
    }
};

static void kf_free(Kf* k)
{
    if (!k) return;
    (void)hipSetDevice(k->device);
    if (k->stream) (void)hipStreamDestroy(k->stream);
    delete k;
}

static Kf* kf_make(const double* time, const double* y, const double* yerr, int n, int p, double sigsqr,
                   const double* omega_re_im, const double* ma, int nma, double car1_omega, int device, const char* who,
                   int* rc_out = nullptr)
{
    int rc_local = CARMA_EINVAL;
    int& rc = rc_out ? *rc_out : rc_local;
    rc = CARMA_EINVAL;
    if (!time || !y || !yerr || n < 1) {
        set_error("%s: bad argument", who);
        return nullptr;
    }
    if (p != 1 && (p < 2 || p > CARMA_PMAX || !omega_re_im || !ma || nma < 1)) {
        set_error("%s: need 2 <= p <= %d, omega and ma", who, CARMA_PMAX);
        return nullptr;
    }
    rc = select_device(device);
    if (rc != CARMA_OK) return nullptr;
    rc = CARMA_EINVAL;
    std::vector<double> t(time, time + n), yy(y, y + n), ee(yerr, yerr + n);
    if (n >= 2) sort_dedup(t, yy, ee);
    std::vector<double> s = pack_series(t, yy, ee);
    std::vector<double> par(2 * CARMA_PMAX + CARMA_PMAX, 0.0);
    if (p > 1) {
        if (pack_model_single(p, omega_re_im, ma, nma, par.data()) != CARMA_OK) {
            set_error("%s: the AR roots must be real or come in complex-conjugate pairs", who);
            return nullptr;
        }
    }
    Kf* k = new Kf();
    k->device = device;
    k->p = p;
    k->n = (int)t.size();
    k->sigsqr = sigsqr;
    k->car1_omega = car1_omega;
    hipError_t e = k->d_series.alloc(sizeof(double) * s.size());
    if (e == hipSuccess) e = k->d_par.alloc(sizeof(double) * par.size());
    if (e == hipSuccess) e = k->d_sing.alloc(sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(k->d_series.as<void>(), s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(k->d_par.as<void>(), par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        rc = hip_fail(e, who);
        kf_free(k);
        return nullptr;
    }
    rc = CARMA_OK;
    return k;
}

// Filter() + GetMean() / GetVar() (kfilter.hpp:126-132)
static int kf_filter(Kf* k, double* mean, double* var)
{
    if (!mean || !var) return CARMA_EINVAL;
    hipError_t e = hipSetDevice(k->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    const int m = k->n;
    int rc = k->ensure_io(2 * (size_t)m);
    if (rc != CARMA_OK) return rc;
    double* d_io = k->d_io.as<double>();
    const double* d_par = k->d_par.as<double>();
    int* d_sing = k->d_sing.as<int>();
    e = hipMemsetAsync(d_sing, 0, sizeof(int), k->stream);
    if (e == hipSuccess) {
        if (k->p == 1)
            e = launch_kfilter_car1(k->sigsqr, k->car1_omega, k->d_series.as<const double4>(), m, d_io, d_io + m, k->stream);
        else
            e = launch_kfilter_carma(k->p, d_par, d_par + 2 * CARMA_PMAX, k->sigsqr, k->d_series.as<const double4>(), m, d_io,
                                     d_io + m, d_sing, k->stream);
    }
    int sing = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(mean, d_io, sizeof(double) * m, hipMemcpyDeviceToHost, k->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(var, d_io + m, sizeof(double) * m, hipMemcpyDeviceToHost, k->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&sing, d_sing, sizeof(int), hipMemcpyDeviceToHost, k->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(k->stream);
    if (e != hipSuccess) {
        // copies enqueued before the failure may still be writing into the caller's buffers (and into `sing` on this
        // stack frame): drain the stream before anybody frees or leaves them
        (void)hipStreamSynchronize(k->stream);
        return hip_fail(e, "carma_kfilter");
    }
    return sing ? 1 : CARMA_OK;
}

// Predict for M times in one launch (kfilter.cpp:218-337, 72-135)
static int kf_predict(Kf* k, const double* tpred, int M, double* pmean, double* pvar)
{
    if (!tpred || !pmean || !pvar || M < 0) {
        set_error("carma_predict: bad argument");
        return CARMA_EINVAL;
    }
    if (M == 0) return CARMA_OK;
    hipError_t e = hipSetDevice(k->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    int rc = k->ensure_io(3 * (size_t)M);
    if (rc != CARMA_OK) return rc;
    double* d_io = k->d_io.as<double>();
    const double* d_par = k->d_par.as<double>();
    int* d_sing = k->d_sing.as<int>();
    e = hipMemcpyAsync(d_io, tpred, sizeof(double) * M, hipMemcpyHostToDevice, k->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_sing, 0, sizeof(int), k->stream);
    if (e == hipSuccess) {
        if (k->p == 1)
            e = launch_predict_car1(k->sigsqr, k->car1_omega, k->d_series.as<const double4>(), k->n, d_io, M, d_io + M,
                                    d_io + 2 * (size_t)M, k->stream);
        else
            e = launch_predict_carma(k->p, d_par, d_par + 2 * CARMA_PMAX, k->sigsqr, k->d_series.as<const double4>(), k->n, d_io, M,
                                     d_io + M, d_io + 2 * (size_t)M, d_sing, k->stream);
    }
    int sing = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(pmean, d_io + M, sizeof(double) * M, hipMemcpyDeviceToHost, k->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(pvar, d_io + 2 * (size_t)M, sizeof(double) * M, hipMemcpyDeviceToHost, k->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&sing, d_sing, sizeof(int), hipMemcpyDeviceToHost, k->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(k->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(k->stream);               // see kf_filter
        return hip_fail(e, "carma_predict");
    }
    return sing ? 1 : CARMA_OK;
}

}  // namespace carma

extern "C" {

carma_kf* carma_kf_create_carma(const double* time, const double* y, const double* yerr, int n, int p, double sigsqr,
                                const double* omega_re_im, const double* ma, int nma, int device)
{
    if (p < 2) {
        set_error("carma_kf_create_carma: need 2 <= p <= %d", CARMA_PMAX);
        return nullptr;
    }
    return reinterpret_cast<carma_kf*>(kf_make(time, y, yerr, n, p, sigsqr, omega_re_im, ma, nma, 0.0, device, "carma_kf_create_carma"));
}

carma_kf* carma_kf_create_car1(const double* time, const double* y, const double* yerr, int n, double sigsqr, double omega, int device)
{
    return reinterpret_cast<carma_kf*>(kf_make(time, y, yerr, n, 1, sigsqr, nullptr, nullptr, 0, omega, device, "carma_kf_create_car1"));
}

void carma_kf_destroy(carma_kf* h) { kf_free(reinterpret_cast<Kf*>(h)); }
int carma_kf_n(const carma_kf* h) { return h ? reinterpret_cast<const Kf*>(h)->n : CARMA_EINVAL; }
int carma_kf_filter(carma_kf* h, double* mean, double* var) { return h ? kf_filter(reinterpret_cast<Kf*>(h), mean, var) : CARMA_EINVAL; }
int carma_kf_predict(carma_kf* h, const double* tpred, int M, double* pmean, double* pvar)
{
    return h ? kf_predict(reinterpret_cast<Kf*>(h), tpred, M, pmean, pvar) : CARMA_EINVAL;
}

int carma_kfilter_carma(const double* time, const double* y, const double* yerr, int n, int p, double sigsqr,
                        const double* omega_re_im, const double* ma, int nma, double* mean, double* var, int* n_out,
                        int device)
{
    int rc0 = CARMA_EINVAL;
    Kf* k = (p >= 2) ? kf_make(time, y, yerr, n, p, sigsqr, omega_re_im, ma, nma, 0.0, device, "carma_kfilter_carma", &rc0) : nullptr;
    if (!k) {
        if (p < 2) set_error("carma_kfilter_carma: need 2 <= p <= %d, omega and ma", CARMA_PMAX);
        return rc0;
    }
    if (n_out) *n_out = k->n;
    const int rc = kf_filter(k, mean, var);
    kf_free(k);
    return rc;
}

int carma_kfilter_batch_carma(const double* time, const double* y, const double* yerr, int n, int p, int nmodels, const double* sigsqr,
                              const double* omega_re_im, const double* ma, int nma, const double* mu, double* mean, double* var,
                              int* singular, int* n_out, int device)
{
    if (!time || !y || !yerr || n < 2 || p < 2 || p > CARMA_PMAX || nmodels < 1 || !sigsqr || !omega_re_im || !ma || nma < 1 ||
        nma > p || !mean || !var) {
        set_error("carma_kfilter_batch_carma: bad argument (n >= 2, 2 <= p <= %d, 1 <= nma <= p, nmodels >= 1)", CARMA_PMAX);
        return CARMA_EINVAL;
    }
    int rc = select_device(device);
    if (rc != CARMA_OK) return rc;
    DevMem b_s, b_par, b_mv, b_mean, b_var, b_sing;
    std::vector<double> t(time, time + n), yy(y, y + n), ee(yerr, yerr + n);
    sort_dedup(t, yy, ee);
    const int m = (int)t.size();
    if (n_out) *n_out = m;
    const std::vector<double> s = pack_series(t, yy, ee);
    const int PW = 3 * p + 2;
    std::vector<double> par((size_t)nmodels * PW, 0.0);
    for (int b = 0; b < nmodels; b++) {
        if (pack_model_row(p, omega_re_im + (size_t)b * 2 * p, ma + (size_t)b * nma, nma, sigsqr[b], mu ? mu[b] : 0.0,
                           par.data() + (size_t)b * PW) != CARMA_OK) {
            set_error("carma_kfilter_batch_carma: model %d: the AR roots must be real or come in complex-conjugate pairs", b);
            return CARMA_EINVAL;
        }
    }
    const size_t nmv = (size_t)2 * m * ((size_t)nmodels + 64), nout = (size_t)nmodels * m;
    hipError_t e = b_s.alloc(sizeof(double) * s.size());
    if (e == hipSuccess) e = b_par.alloc(sizeof(double) * par.size());
    if (e == hipSuccess) e = b_mv.alloc(sizeof(double) * nmv);
    if (e == hipSuccess) e = b_mean.alloc(sizeof(double) * nout);
    if (e == hipSuccess) e = b_var.alloc(sizeof(double) * nout);
    if (e == hipSuccess) e = b_sing.alloc(sizeof(int) * nmodels);
    double *d_s = b_s.as<double>(), *d_par = b_par.as<double>(), *d_mv = b_mv.as<double>(), *d_mean = b_mean.as<double>(),
           *d_var = b_var.as<double>();
    int* d_sing = b_sing.as<int>();
    if (e == hipSuccess) e = hipMemcpy(d_s, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = launch_kfilter_batch(p, d_par, nmodels, reinterpret_cast<const double4*>(d_s), m, d_mv, d_sing, d_mean, d_var, nullptr);
    if (e == hipSuccess) e = hipMemcpy(mean, d_mean, sizeof(double) * nout, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(var, d_var, sizeof(double) * nout, hipMemcpyDeviceToHost);
    if (e == hipSuccess && singular) e = hipMemcpy(singular, d_sing, sizeof(int) * nmodels, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "carma_kfilter_batch_carma");
    return CARMA_OK;
}

int carma_kfilter_car1(const double* time, const double* y, const double* yerr, int n, double sigsqr, double omega,
                       double* mean, double* var, int* n_out, int device)
{
    int rc0 = CARMA_EINVAL;
    Kf* k = kf_make(time, y, yerr, n, 1, sigsqr, nullptr, nullptr, 0, omega, device, "carma_kfilter_car1", &rc0);
    if (!k) return rc0;
    if (n_out) *n_out = k->n;
    const int rc = kf_filter(k, mean, var);
    kf_free(k);
    return rc;
}

int carma_predict_carma(const double* time, const double* y, const double* yerr, int n, int p, double sigsqr,
                        const double* omega_re_im, const double* ma, int nma, const double* tpred, int M, double* pmean,
                        double* pvar, int device)
{
    int rc0 = CARMA_EINVAL;
    Kf* k = (p >= 2) ? kf_make(time, y, yerr, n, p, sigsqr, omega_re_im, ma, nma, 0.0, device, "carma_predict_carma", &rc0) : nullptr;
    if (!k) {
        if (p < 2) set_error("carma_predict_carma: need 2 <= p <= %d, omega and ma", CARMA_PMAX);
        return rc0;
    }
    const int rc = kf_predict(k, tpred, M, pmean, pvar);
    kf_free(k);
    return rc;
}

int carma_predict_car1(const double* time, const double* y, const double* yerr, int n, double sigsqr, double omega,
                       const double* tpred, int M, double* pmean, double* pvar, int device)
{
    int rc0 = CARMA_EINVAL;
    Kf* k = kf_make(time, y, yerr, n, 1, sigsqr, nullptr, nullptr, 0, omega, device, "carma_predict_car1", &rc0);
    if (!k) return rc0;
    const int rc = kf_predict(k, tpred, M, pmean, pvar);
    kf_free(k);
    return rc;
}

// carma_process / car1_process for npaths paths in one launch
static int simulate_common(const double* time, int n, int p, double sigsqr, const double* omega_re_im, const double* ma,
                           int nma, double car1_omega, int npaths, uint64_t seed, double* out, int device)
{
    if (!time || !out || n < 1 || npaths < 0) {
        set_error("carma_simulate: bad argument");
        return CARMA_EINVAL;
    }
    if (npaths == 0) return CARMA_OK;
    int rc = select_device(device);
    if (rc != CARMA_OK) return rc;
    DevMem b_t, b_par, b_out, b_sing;
    std::vector<double> t(time, time + n);
    std::sort(t.begin(), t.end());                            // time.sort() (carma_pack.py:1176)
    std::vector<double> par(2 * CARMA_PMAX + CARMA_PMAX, 0.0);
    if (p > 1 && pack_model_single(p, omega_re_im, ma, nma, par.data()) != CARMA_OK) {
        set_error("carma_simulate_carma: the AR roots must be real or come in complex-conjugate pairs");
        return CARMA_EINVAL;
    }
    const size_t nout = (size_t)npaths * n;
    hipError_t e = b_t.alloc(sizeof(double) * n);
    if (e == hipSuccess) e = b_par.alloc(sizeof(double) * par.size());
    if (e == hipSuccess) e = b_out.alloc(sizeof(double) * nout);
    if (e == hipSuccess) e = b_sing.alloc(sizeof(int));
    double *d_t = b_t.as<double>(), *d_par = b_par.as<double>(), *d_out = b_out.as<double>();
    int* d_sing = b_sing.as<int>();
    if (e == hipSuccess) e = hipMemcpy(d_t, t.data(), sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_sing, 0, sizeof(int));
    const unsigned s0 = (unsigned)(seed & 0xffffffffu), s1 = (unsigned)(seed >> 32);
    if (e == hipSuccess) {
        if (p == 1)
            e = launch_simulate_car1(sigsqr, car1_omega, d_t, n, npaths, s0, s1, 0u, d_out, nullptr);
        else
            e = launch_simulate_carma(p, d_par, d_par + 2 * CARMA_PMAX, sigsqr, d_t, n, npaths, s0, s1, 0u, d_out, d_sing, nullptr);
    }
    int sing = 0;
    if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(double) * nout, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&sing, d_sing, sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "carma_simulate");
    return sing ? 1 : CARMA_OK;
}

int carma_simulate_carma(const double* time, int n, int p, double sigsqr, const double* omega_re_im, const double* ma, int nma,
                         int npaths, uint64_t seed, double* out, int device)
{
    if (p < 2 || p > CARMA_PMAX || !omega_re_im || !ma || nma < 1 || !(sigsqr > 0.0)) {
        set_error("carma_simulate_carma: need 2 <= p <= %d, omega, ma and sigsqr > 0", CARMA_PMAX);
        return CARMA_EINVAL;
    }
    return simulate_common(time, n, p, sigsqr, omega_re_im, ma, nma, 0.0, npaths, seed, out, device);
}

int carma_simulate_car1(const double* time, int n, double sigsqr, double omega, int npaths, uint64_t seed, double* out, int device)
{
    if (!(sigsqr > 0.0) || !(omega > 0.0)) {
        set_error("carma_simulate_car1: need sigsqr > 0 and omega > 0");
        return CARMA_EINVAL;
    }
    return simulate_common(time, n, 1, sigsqr, nullptr, nullptr, 0, omega, npaths, seed, out, device);
}

}  // extern "C"
