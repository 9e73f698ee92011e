// hostmem_main.cpp -- TEST HARNESS ONLY: the buffer owners (carma_pack_amd/csrc/carma_devbuf.h), the buffer requests of the sampler
// states (carma_pt_state.h) and the model-row packers (carma_model_pack.h) of the host layer as a stand-alone program without the
// HIP runtime and without Python: the form in which they can run under the host sanitizers (g++ -fsanitize=address,undefined).
// tests/test_hostmem_cpu.py builds and runs it plain.
// carma_dev_malloc / carma_dev_free and carma_pinned_malloc / carma_pinned_free are defined HERE, over malloc / free: they record
// every request and every release, and can be told to fail the k-th request.
// Usage: hostmem_main [group]; no argument runs every group.  Exit status 0: every check met; 1: the first miss, named on stderr.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "carma_devbuf.h"
#include "carma_model_pack.h"
#include "carma_pt_state.h"

#define CHECK(cond, ...)                                                           \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "MISS %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                     \
            std::fprintf(stderr, "\n");                                            \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

namespace {
struct Event {
    char kind;                  // 'M': a device request (n = its size; p = null when it was failed), 'F': a device release;
                                // 'H' / 'G': the same of pinned host memory
    size_t n;
    void* p;
};
std::vector<Event> g_log;
std::map<void*, size_t> g_live;
std::map<void*, char> g_kind;   // of every live block: the kind of its request
long g_fail_in = 0;             // > 0: the g_fail_in-th request from now (of either kind) fails
int g_poison;                   // a failed request leaves this address in *p: the owner must not keep it

void reset()
{
    CHECK(g_live.empty(), "%zu allocation(s) were never released", g_live.size());
    g_log.clear();
    g_fail_in = 0;
}
std::vector<size_t> requests()
{
    std::vector<size_t> r;
    for (const Event& e : g_log)
        if (e.kind == 'M') r.push_back(e.n);
    return r;
}
size_t count_kind(char kind)
{
    size_t k = 0;
    for (const Event& e : g_log) k += e.kind == kind;
    return k;
}
size_t frees() { return count_kind('F'); }

hipError_t record_malloc(char kind, void** p, size_t n)
{
    if (g_fail_in > 0 && --g_fail_in == 0) {
        g_log.push_back({kind, n, nullptr});
        *p = &g_poison;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(n ? n : 1);
    CHECK(*p, "malloc(%zu)", n);
    g_live[*p] = n;
    g_kind[*p] = kind;
    g_log.push_back({kind, n, *p});
    return hipSuccess;
}
hipError_t record_free(char kind, char kind_of_request, void* p)
{
    CHECK(p, "release of a null pointer reached the allocator");
    CHECK(g_live.count(p) == 1, "release of %p, which is not live (released twice, or never allocated)", p);
    CHECK(g_kind[p] == kind_of_request, "%p was requested as '%c' and is released as '%c'", p, g_kind[p], kind);
    g_live.erase(p);
    g_kind.erase(p);
    g_log.push_back({kind, 0, p});
    std::free(p);
    return hipSuccess;
}
}  // namespace

hipError_t carma_dev_malloc(void** p, size_t n) { return record_malloc('M', p, n); }
hipError_t carma_dev_free(void* p) { return record_free('F', 'M', p); }
hipError_t carma_pinned_malloc(void** p, size_t n) { return record_malloc('H', p, n); }
hipError_t carma_pinned_free(void* p) { return record_free('G', 'H', p); }

namespace {
using carma::DevMem;

void devmem_alloc()
{
    reset();
    {
        DevMem m;
        CHECK(m.as<void>() == nullptr && m.capacity() == 0, "a new DevMem is not empty");
        CHECK(m.alloc(24) == hipSuccess, "alloc(24)");
        CHECK((requests() == std::vector<size_t>{24}), "alloc(24) did not request exactly 24 bytes");
        CHECK(m.capacity() == 24 && m.as<double>() != nullptr, "capacity %zu", m.capacity());
        void* first = m.as<void>();
        std::memset(first, 0x5a, 24);                                      // (the sanitizer build checks the extent)
        CHECK(m.alloc(7) == hipSuccess, "alloc(7)");
        CHECK(g_log.size() == 3 && g_log[1].kind == 'F' && g_log[1].p == first && g_log[2].kind == 'M' && g_log[2].n == 7,
              "the second alloc did not release the first block before its request");
        CHECK(m.capacity() == 7 && g_live.size() == 1, "capacity %zu, %zu live", m.capacity(), g_live.size());
    }
    CHECK(g_live.empty() && frees() == 2, "the destructor did not release (%zu live, %zu releases)", g_live.size(), frees());
    reset();
    {
        DevMem m;
        CHECK(m.alloc(100) == hipSuccess, "alloc(100)");
        m.release();
        CHECK(g_live.empty() && m.as<void>() == nullptr && m.capacity() == 0, "release() left something behind");
        m.release();                                                       // idempotent
        CHECK(frees() == 1, "%zu releases after two release() calls", frees());
    }
    CHECK(frees() == 1, "the destructor released again after release() (%zu releases)", frees());
    reset();
    {
        DevMem a, c;
        CHECK(a.alloc(10) == hipSuccess && c.alloc(30) == hipSuccess, "alloc");
        void *pa = a.as<void>(), *pc = c.as<void>();
        DevMem b(std::move(a));                                            // move construction
        CHECK(a.as<void>() == nullptr && a.capacity() == 0, "the source of a move construction is not empty");
        CHECK(b.as<void>() == pa && b.capacity() == 10 && frees() == 0, "move construction");
        c = std::move(b);                                                  // move assignment: c's block goes, b's arrives
        CHECK(b.as<void>() == nullptr && b.capacity() == 0, "the source of a move assignment is not empty");
        CHECK(c.as<void>() == pa && c.capacity() == 10, "move assignment");
        CHECK(frees() == 1 && g_log.back().kind == 'F' && g_log.back().p == pc, "move assignment did not release the target's block");
        c = std::move(c);                                                  // onto itself: nothing happens
        CHECK(c.as<void>() == pa && frees() == 1, "self move assignment");
    }
    CHECK(g_live.empty() && frees() == 2, "after the moves: %zu live, %zu releases for 2 allocations", g_live.size(), frees());
    reset();
    {
        DevMem m;
        CHECK(m.alloc(16) == hipSuccess, "alloc(16)");
        g_fail_in = 1;
        CHECK(m.alloc(32) == hipErrorOutOfMemory, "a failed request was not reported");
        CHECK(m.as<void>() == nullptr && m.capacity() == 0, "not empty after a failed request");
        CHECK(g_live.empty(), "the old block outlived a failed alloc");
        CHECK(m.alloc(0) == hipSuccess && requests().back() == 0 && m.capacity() == 0, "a request of 0 bytes is passed on as 0 bytes");
    }
    CHECK(g_live.empty(), "leak");
    reset();
}

void devmem_need()
{
    reset();
    {
        DevMem m;
        const size_t ask[] = {1, 4096, 4097, 5000, 10000, 100}, want[] = {4096, 0, 5121, 0, 12500, 0}, cap[] = {4096, 4096, 5121, 5121, 12500, 12500};
        for (int i = 0; i < 6; i++) {
            const size_t nreq = requests().size(), nfree = frees(), nlog = g_log.size();
            void* before = m.as<void>();
            CHECK(m.need(ask[i]) == hipSuccess, "need(%zu)", ask[i]);
            if (want[i] == 0) {
                CHECK(g_log.size() == nlog && m.as<void>() == before, "need(%zu) touched the allocator", ask[i]);
            } else {
                CHECK(requests().size() == nreq + 1 && requests().back() == want[i], "need(%zu) requested %zu bytes, not %zu", ask[i],
                      requests().back(), want[i]);
                if (before)
                    CHECK(frees() == nfree + 1 && g_log[nlog].kind == 'F' && g_log[nlog].p == before && g_log[nlog + 1].kind == 'M',
                          "need(%zu): the old block was not released before the new request", ask[i]);
            }
            CHECK(m.capacity() == cap[i] && g_live.size() == 1, "need(%zu): capacity %zu, %zu live", ask[i], m.capacity(), g_live.size());
        }
        g_fail_in = 1;
        CHECK(m.need(20000) == hipErrorOutOfMemory, "a failed growth was not reported");
        CHECK(requests().back() == 25000, "need(20000) requested %zu", requests().back());
        CHECK(m.as<void>() == nullptr && m.capacity() == 0 && g_live.empty(), "not empty after a failed growth");
        CHECK(m.need(8) == hipSuccess && m.capacity() == 4096, "need after a failed growth");
    }
    CHECK(g_live.empty(), "leak");
    reset();
}

constexpr double GUARD = -777.25;
const double ULP_RE = std::nextafter(-0.3, 0.0);

struct RootCase {
    const char* what;
    int p, rc;
    std::vector<double> in, out;
};

// the expected order, by hand: every pair as (re, -|im|), (re, +|im|) in the order its first member appears; real roots last, in
// input order
const std::vector<RootCase>& root_cases()
{
    static const std::vector<RootCase> c = {
        {"p=1 real", 1, CARMA_OK, {-0.5, 0}, {-0.5, 0}},
        {"p=1 lone complex", 1, CARMA_EINVAL, {-0.5, 0.3}, {}},
        {"p=2 pair adjacent", 2, CARMA_OK, {-1, -2, -1, 2}, {-1, -2, -1, 2}},
        {"p=2 positive first", 2, CARMA_OK, {-1, 2, -1, -2}, {-1, -2, -1, 2}},
        {"p=2 two real", 2, CARMA_OK, {-1, 0, -3, 0}, {-1, 0, -3, 0}},
        {"p=2 lone complex", 2, CARMA_EINVAL, {-1, 2, -3, 0}, {}},
        {"p=3 real inside the pair", 3, CARMA_OK, {-1, 2, -5, 0, -1, -2}, {-1, -2, -1, 2, -5, 0}},
        {"p=3 lone complex", 3, CARMA_EINVAL, {-5, 0, -1, -2, -6, 0}, {}},
        {"p=4 pairs split apart", 4, CARMA_OK, {-1, 2, -3, -4, -1, -2, -3, 4}, {-1, -2, -1, 2, -3, -4, -3, 4}},
        {"p=4 pairs adjacent", 4, CARMA_OK, {-3, -4, -3, 4, -1, -2, -1, 2}, {-3, -4, -3, 4, -1, -2, -1, 2}},
        {"p=4 conjugate of the wrong root", 4, CARMA_EINVAL, {-1, 2, -3, -4, -1, -2, -3.5, 4}, {}},
        {"p=5 real roots around the pair", 5, CARMA_OK, {-7, 0, -1, -2, -8, 0, -1, 2, -9, 0}, {-1, -2, -1, 2, -7, 0, -8, 0, -9, 0}},
        {"p=5 two pairs, real between", 5, CARMA_OK, {-1, 2, -3, 4, -6, 0, -3, -4, -1, -2}, {-1, -2, -1, 2, -3, -4, -3, 4, -6, 0}},
        {"p=5 lone complex", 5, CARMA_EINVAL, {-7, 0, -1, -2, -8, 0, -1, 2, -9, 1}, {}},
        {"p=6 mate one ulp off",
         6,
         CARMA_OK,
         {-0.3, 0.7, -2, 0, ULP_RE, -0.7, -4, 5, -1, 0, -4, -5},
         {-0.3, -0.7, -0.3, 0.7, -4, -5, -4, 5, -2, 0, -1, 0}},
        {"p=6 three pairs adjacent", 6, CARMA_OK, {-1, -1, -1, 1, -2, -2, -2, 2, -3, -3, -3, 3}, {-1, -1, -1, 1, -2, -2, -2, 2, -3, -3, -3, 3}},
        {"p=6 mate off by 1e-9", 6, CARMA_EINVAL, {-0.3, 0.7, -2, 0, -0.3 + 1e-9, -0.7, -4, 5, -1, 0, -4, -5}, {}},
        {"p=7 positive first, real in the middle",
         7,
         CARMA_OK,
         {-1, 1, -1, -1, -2, 2, -6, 0, -2, -2, -3, -3, -3, 3},
         {-1, -1, -1, 1, -2, -2, -2, 2, -3, -3, -3, 3, -6, 0}},
        {"p=7 all real", 7, CARMA_OK, {-7, 0, -6, 0, -5, 0, -4, 0, -3, 0, -2, 0, -1, 0}, {-7, 0, -6, 0, -5, 0, -4, 0, -3, 0, -2, 0, -1, 0}},
        {"p=7 lone complex", 7, CARMA_EINVAL, {-1, 1, -1, -1, -2, 2, -6, 0, -2, -2, -3, -3, -3, 3.1}, {}},
    };
    return c;
}

void roots()
{
    bool seen[8] = {false};
    for (const RootCase& c : root_cases()) {
        CHECK((int)c.in.size() == 2 * c.p, "%s: the case itself is malformed", c.what);
        seen[c.p] = true;
        std::vector<double> out(2 * c.p + 4, GUARD);
        const int rc = carma::normalize_roots(c.p, c.in.data(), out.data());
        CHECK(rc == c.rc, "%s: rc %d, expected %d", c.what, rc, c.rc);
        for (int i = 2 * c.p; i < 2 * c.p + 4; i++) CHECK(out[i] == GUARD, "%s: wrote past the %d roots (slot %d)", c.what, c.p, i);
        if (rc != CARMA_OK) continue;
        for (int i = 0; i < 2 * c.p; i++)
            CHECK(out[i] == c.out[i] && std::signbit(out[i]) == std::signbit(c.out[i]), "%s: out[%d] = %.17g, expected %.17g", c.what, i,
                  out[i], c.out[i]);
    }
    for (int p = 1; p <= 7; p++) CHECK(seen[p], "no case for p = %d", p);
}

const double MA7[7] = {1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625};

struct RowCase {
    int p;
    std::vector<double> in, roots;      // as given; as the kernels read them
};
const std::vector<RowCase>& row_cases()
{
    static const std::vector<RowCase> c = {
        {2, {-1, 2, -1, -2}, {-1, -2, -1, 2}},
        {3, {-1, 2, -5, 0, -1, -2}, {-1, -2, -1, 2, -5, 0}},
        {7, {-1, 1, -1, -1, -2, 2, -6, 0, -2, -2, -3, -3, -3, 3}, {-1, -1, -1, 1, -2, -2, -2, 2, -3, -3, -3, 3, -6, 0}},
    };
    return c;
}

void expect_eq(const char* what, int p, int nma, const std::vector<double>& got, const std::vector<double>& want)
{
    CHECK(got.size() == want.size(), "%s p=%d nma=%d: the case itself is malformed", what, p, nma);
    for (size_t i = 0; i < want.size(); i++)
        CHECK(got[i] == want[i] && std::signbit(got[i]) == std::signbit(want[i]), "%s p=%d nma=%d: slot %zu = %.17g, expected %.17g", what,
              p, nma, i, got[i], want[i]);
}

void rows()
{
    const double sigsqr = 2.5, mu = -0.75;
    // two rows in full, as a reader would write them down
    {
        std::vector<double> row(8 + 2, 99.0);
        CHECK(carma::pack_model_row(2, row_cases()[0].in.data(), MA7, 1, sigsqr, mu, row.data()) == CARMA_OK, "p=2 nma=1");
        expect_eq("row", 2, 1, row, {-1, -2, -1, 2, 1.0, 0.0, 2.5, -0.75, 99.0, 99.0});
        std::vector<double> row3(11 + 2, 99.0);
        CHECK(carma::pack_model_row(3, row_cases()[1].in.data(), MA7, 2, sigsqr, mu, row3.data()) == CARMA_OK, "p=3 nma=2");
        expect_eq("row", 3, 2, row3, {-1, -2, -1, 2, -5, 0, 1.0, 0.5, 0.0, 2.5, -0.75, 99.0, 99.0});
        std::vector<double> par(21 + 2, 99.0);
        CHECK(carma::pack_model_single(3, row_cases()[1].in.data(), MA7, 2, par.data()) == CARMA_OK, "single p=3 nma=2");
        expect_eq("single", 3, 2, par, {-1, -2, -1, 2, -5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0.5, 0, 0, 0, 0, 0, 99.0, 99.0});
    }
    for (const RowCase& c : row_cases()) {
        const int p = c.p, W = 3 * p + 2;
        for (int nma : {1, p - 1, p}) {
            // [2 p roots][ma[0 .. nma), zeros to p][sigsqr][mu]; the row arrives pre-filled, two guard slots behind it
            std::vector<double> want(c.roots);
            for (int i = 0; i < p; i++) want.push_back(i < nma ? MA7[i] : 0.0);
            want.insert(want.end(), {sigsqr, mu, GUARD, GUARD});
            std::vector<double> row(W, 99.0);
            row.insert(row.end(), {GUARD, GUARD});
            CHECK(carma::pack_model_row(p, c.in.data(), MA7, nma, sigsqr, mu, row.data()) == CARMA_OK, "p=%d nma=%d", p, nma);
            expect_eq("row", p, nma, row, want);
        }
        for (int nma : {1, p - 1, p, p + 2}) {
            // [2 CARMA_PMAX: 2 p roots, zeros][CARMA_PMAX: the first min(p, nma) coefficients, zeros]
            std::vector<double> want(c.roots);
            want.resize(2 * CARMA_PMAX, 0.0);
            for (int i = 0; i < CARMA_PMAX; i++) want.push_back(i < nma && i < p ? MA7[i] : 0.0);
            want.insert(want.end(), {GUARD, GUARD});
            std::vector<double> par(3 * CARMA_PMAX, 99.0);
            par.insert(par.end(), {GUARD, GUARD});
            if (nma > 7) continue;                                        // (MA7 holds seven)
            CHECK(carma::pack_model_single(p, c.in.data(), MA7, nma, par.data()) == CARMA_OK, "single p=%d nma=%d", p, nma);
            expect_eq("single", p, nma, par, want);
        }
    }
    // open roots: CARMA_EINVAL, nothing written behind the row
    const double open3[6] = {-1, 2, -5, 0, -1, -2.5};
    std::vector<double> row(11, 99.0), par(21, 99.0);
    row.insert(row.end(), {GUARD, GUARD});
    par.insert(par.end(), {GUARD, GUARD});
    CHECK(carma::pack_model_row(3, open3, MA7, 3, sigsqr, mu, row.data()) == CARMA_EINVAL, "open roots: row");
    CHECK(carma::pack_model_single(3, open3, MA7, 3, par.data()) == CARMA_EINVAL, "open roots: single");
    CHECK(row[11] == GUARD && row[12] == GUARD && par[21] == GUARD && par[22] == GUARD, "open roots: wrote behind the row");
}

// ---- the typed owners (DevBuf<T>, PinnedBuf<T>) -----------------------------------------------------------------------------
// Buf: an owner of doubles; req / rel: the kinds its requests and releases are recorded as
template <class Buf>
void typed_owner(const char* what, char req, char rel)
{
    reset();
    {
        Buf b;
        CHECK(b.get() == nullptr && !b, "%s: a new owner is not empty", what);
        CHECK(b.alloc(5) == hipSuccess, "%s: alloc(5)", what);
        CHECK(g_log.size() == 1 && g_log[0].kind == req && g_log[0].n == 40, "%s: alloc(5) is not one request of 40 bytes", what);
        double* p = b;                                                     // conversion
        const double* cp = b;
        void* vp = b;
        CHECK(p && p == b.get() && cp == p && vp == p && b, "%s: conversion to a pointer", what);
        CHECK(b + 2 == p + 2 && &b[3] == p + 3, "%s: pointer arithmetic", what);
        for (int i = 0; i < 5; i++) b[i] = i;                              // (the sanitizer build checks the extent)
        double copy[5];
        std::memcpy(copy, b, 40);                                          // (as hipMemcpy takes it: void*)
        std::memcpy(b, copy, 40);
        Buf m(std::move(b));                                               // move construction
        CHECK(!b && b.get() == nullptr && m.get() == p && count_kind(rel) == 0, "%s: move construction", what);
        Buf c;
        CHECK(c.alloc(2) == hipSuccess, "%s: alloc(2)", what);
        double* pc = c;
        c = std::move(m);                                                  // move assignment: c's block goes, m's arrives
        CHECK(!m && c.get() == p && count_kind(rel) == 1 && g_log.back().kind == rel && g_log.back().p == pc, "%s: move assignment", what);
        g_fail_in = 1;
        CHECK(c.alloc(7) == hipErrorOutOfMemory, "%s: a failed request was not reported", what);
        CHECK(!c && c.get() == nullptr && g_live.empty(), "%s: not empty after a failed request", what);
        CHECK(c.alloc(3) == hipSuccess && g_log.back().n == 24, "%s: alloc after a failed request", what);
        c.release();
        c.release();                                                       // idempotent
        CHECK(!c && g_live.empty(), "%s: release()", what);
        CHECK(c.alloc(1) == hipSuccess, "%s: alloc(1)", what);             // ... and the destructor releases this one
    }
    CHECK(g_live.empty() && count_kind(req) == 5 && count_kind(rel) == 4, "%s: %zu requests (one failed), %zu releases", what,
          count_kind(req), count_kind(rel));
    CHECK(g_log.size() == count_kind(req) + count_kind(rel), "%s touched the other allocator", what);
    reset();
}

void typed_buf()
{
    typed_owner<carma::DevBuf<double>>("DevBuf", 'M', 'F');
    carma::DevBuf<char> c;                                                 // bytes = count * sizeof(T)
    carma::DevBuf<unsigned long long> u;
    CHECK(c.alloc(3) == hipSuccess && u.alloc(3) == hipSuccess, "alloc");
    CHECK((requests() == std::vector<size_t>{3, 24}), "element counts of char and unsigned long long");
}

void pinned_buf() { typed_owner<carma::PinnedBuf<double>>("PinnedBuf", 'H', 'G'); }

// ---- the buffer requests of the sampler states (carma_pt_state.h) -------------------------------------------------------------
constexpr int ENS_T = 3, ENS_R = 2, ENS_D = 5;
constexpr size_t ENS_NC = (size_t)ENS_T * ENS_R, ENS_SCRATCH = 777, ENS_SERIES = 4;

// One sampler family: a create requests the ensemble's six buffers and then the family's (`extra`, in bytes), as carma_pt_create /
// carma_mpt_create do; the state is deleted as the library deletes it.  Every request failed in turn.
template <class S, class F>
void ensemble_family(const char* name, const std::vector<size_t>& extra, F family)
{
    std::vector<size_t> want = {8 * ENS_T, 8 * ENS_NC * ENS_D, 8 * ENS_NC, 8 * ENS_NC * ENS_D * ENS_D, 4 * ENS_NC, 4 * ENS_NC};
    want.insert(want.end(), extra.begin(), extra.end());
    auto create = [&](hipError_t* e) {
        std::unique_ptr<S> s(new S());
        *e = s->reserve(ENS_T, ENS_R, ENS_D);
        if (*e == hipSuccess) *e = family(s.get());
        return s;
    };
    hipError_t e = hipSuccess;
    reset();
    {
        const std::unique_ptr<S> s = create(&e);
        CHECK(e == hipSuccess, "%s: create", name);
        CHECK(requests() == want, "%s: the requests of a create are not the expected %zu, in bytes and order", name, want.size());
        CHECK(s->T == ENS_T && s->R == ENS_R && s->nchain() == ENS_NC, "%s: T, R", name);
        CHECK(s->d_theta && s->d_theta == s->own_theta.get() && s->d_lp && s->d_lp == s->own_lp.get(), "%s: the views show the own buffers", name);
        CHECK(g_live.size() == want.size() && frees() == 0, "%s: %zu live", name, g_live.size());
    }
    CHECK(g_live.empty() && frees() == want.size(), "%s: deleting the state released %zu of %zu", name, frees(), want.size());
    for (size_t k = 1; k <= want.size(); k++) {
        reset();
        g_fail_in = (long)k;
        {
            const std::unique_ptr<S> s = create(&e);
            CHECK(e == hipErrorOutOfMemory, "%s: request %zu failed and the create did not report it", name, k);
            CHECK(requests().size() == k && g_live.size() == k - 1, "%s: request %zu failed: %zu requests, %zu live", name, k,
                  requests().size(), g_live.size());
        }
        CHECK(g_live.empty() && frees() == k - 1, "%s: request %zu failed: %zu releases for %zu buffers", name, k, frees(), k - 1);
    }
    reset();
}

void ensemble()
{
    using carma::MptState;
    using carma::PtState;
    ensemble_family<PtState>("ladder", {}, [](PtState*) { return hipSuccess; });
    ensemble_family<PtState>("row", {8 * 4 * ENS_NC * (ENS_D + 1), 4, 8 * ENS_NC * (ENS_D + 1 + ENS_D * ENS_D)},
                             [](PtState* s) { return s->reserve_row(ENS_D); });
    ensemble_family<PtState>("lane", {8 * ENS_SCRATCH}, [](PtState* s) { return s->d_scratch.alloc(ENS_SCRATCH); });
    ensemble_family<MptState>("multi-series", {4 * (size_t)ENS_R, ENS_SERIES, 8 * ENS_SCRATCH},
                              [](MptState* s) {
                                  hipError_t e = s->d_lser.alloc((size_t)ENS_R);
                                  if (e == hipSuccess) e = s->d_rep.alloc(ENS_SERIES);
                                  if (e == hipSuccess) e = s->d_scratch.alloc(ENS_SCRATCH);
                                  return e;
                              });
}

// reserve 8, then 3, then 20 samples per ladder: two pairs of requests; a failed second request of a pair leaves nothing
void samples()
{
    reset();
    {
        carma::PtEnsemble s;
        CHECK(s.reserve(ENS_T, ENS_R, ENS_D) == hipSuccess, "reserve");
        const size_t n0 = requests().size();
        const int ask[3] = {8, 3, 20};
        const long holds[3] = {8, 8, 20};
        for (int i = 0; i < 3; i++) {
            long capacity = -1;
            CHECK(s.reserve_samples(ENS_D, ask[i], &capacity) == hipSuccess, "reserve_samples(%d)", ask[i]);
            CHECK(capacity == holds[i] && s.cap == ask[i], "reserve_samples(%d): capacity %ld, stride %ld", ask[i], capacity, s.cap);
            CHECK(s.d_samples && s.d_slp, "reserve_samples(%d): no buffers", ask[i]);
            s.cap = capacity;                                              // (the end of a sampling call)
        }
        const std::vector<size_t> r = requests();
        CHECK((std::vector<size_t>(r.begin() + n0, r.end()) ==
               std::vector<size_t>{8 * ENS_R * 8 * ENS_D, 8 * ENS_R * 8, 8 * ENS_R * 20 * ENS_D, 8 * ENS_R * 20}),
              "8, 3, 20 samples did not give exactly two pairs of requests of R ns d 8 and R ns 8 bytes");
        CHECK(frees() == 2 && g_live.size() == n0 + 2, "the first pair was not released for the second");
        // the second request of a pair fails
        g_fail_in = 2;
        long capacity = -1;
        CHECK(s.reserve_samples(ENS_D, 50, &capacity) == hipErrorOutOfMemory, "a failed request was not reported");
        CHECK(s.cap == 0 && !s.d_samples && !s.d_slp && g_live.size() == n0, "after the failure: cap %ld, %zu live (want %zu)", s.cap,
              g_live.size(), n0);
        const size_t n1 = requests().size();
        CHECK(s.reserve_samples(ENS_D, 2, &capacity) == hipSuccess && capacity == 2, "reserve after a failure");
        CHECK(requests().size() == n1 + 2 && requests()[n1] == 8 * ENS_R * 2 * ENS_D && requests()[n1 + 1] == 8 * ENS_R * 2,
              "the reserve after a failure did not ask for both buffers again");
        // ... and the first
        g_fail_in = 1;
        CHECK(s.reserve_samples(ENS_D, 60, &capacity) == hipErrorOutOfMemory, "a failed first request was not reported");
        CHECK(s.cap == 0 && !s.d_samples && !s.d_slp && g_live.size() == n0, "after a failed first request");
    }
    CHECK(g_live.empty(), "leak");
    reset();
}

// the four boundary buffers of the sharded ladder: all or none
void boundary()
{
    const size_t nbuf = (size_t)ENS_R * (ENS_D + 1) + 1;
    const std::vector<size_t> want = {8 * nbuf, 8 * nbuf, 4, 32};
    reset();
    {
        carma::PtState s;
        CHECK(s.reserve(ENS_T, ENS_R, ENS_D) == hipSuccess, "reserve");
        const size_t live0 = g_live.size();
        for (long k = 1; k <= 4; k++) {
            const size_t n0 = requests().size();
            g_fail_in = k;
            CHECK(s.reserve_boundary(nbuf) == hipErrorOutOfMemory, "boundary request %ld failed and was not reported", k);
            CHECK(requests().size() == n0 + (size_t)k, "boundary request %ld failed: %zu requests", k, requests().size() - n0);
            CHECK(!s.d_send && !s.d_recv && !s.d_bnd_swaps && !s.d_checksum && g_live.size() == live0,
                  "boundary request %ld failed: something is still held (%zu live, want %zu)", k, g_live.size(), live0);
        }
        const size_t n0 = requests().size();
        CHECK(s.reserve_boundary(nbuf) == hipSuccess, "reserve_boundary");
        const std::vector<size_t> r = requests();
        CHECK(std::vector<size_t>(r.begin() + n0, r.end()) == want, "the reserve after the failures did not ask for all four again");
        CHECK(s.d_send && s.d_recv && s.d_bnd_swaps && s.d_checksum && g_live.size() == live0 + 4, "the four buffers");
        s.release_boundary();
        CHECK(!s.d_send && g_live.size() == live0, "release_boundary");
        CHECK(s.reserve_boundary(nbuf) == hipSuccess, "reserve_boundary again");
    }
    CHECK(g_live.empty(), "leak");
    reset();
}

// carma_pt_bind_state: the caller's memory takes the place of the library's two buffers and never reaches the allocator
void bind()
{
    static double ext_theta[ENS_NC * ENS_D], ext_lp[ENS_NC], ext_theta2[ENS_NC * ENS_D], ext_lp2[ENS_NC];
    reset();
    {
        std::unique_ptr<carma::PtState> s(new carma::PtState());
        CHECK(s->reserve(ENS_T, ENS_R, ENS_D) == hipSuccess, "reserve");
        void *own_t = s->own_theta.get(), *own_l = s->own_lp.get();
        s->bind(ext_theta, ext_lp);
        CHECK(s->d_theta == ext_theta && s->d_lp == ext_lp && !s->own_theta && !s->own_lp, "bind: the views and the owners");
        CHECK(frees() == 2 && g_log[g_log.size() - 2].p == own_t && g_log.back().p == own_l, "bind did not release the library's two buffers");
        s->bind(ext_theta2, ext_lp2);                                      // a second bind: the first caller's memory is left alone
        CHECK(s->d_theta == ext_theta2 && s->d_lp == ext_lp2 && frees() == 2, "second bind");
    }
    // (a release of the caller's memory would have stopped the program in record_free: it is not live)
    CHECK(g_live.empty() && frees() == 6, "bound state deleted: %zu releases for 6 buffers", frees());
    for (const Event& e : g_log)
        CHECK(e.p != ext_theta && e.p != ext_lp && e.p != ext_theta2 && e.p != ext_lp2, "the caller's memory reached the allocator");
    reset();
}

const struct { const char* name; void (*run)(); } GROUPS[] = {
    {"devmem_alloc", devmem_alloc}, {"devmem_need", devmem_need}, {"roots", roots}, {"rows", rows}, {"typed_buf", typed_buf},
    {"pinned_buf", pinned_buf}, {"ensemble", ensemble}, {"samples", samples}, {"boundary", boundary}, {"bind", bind}};

}  // namespace

int main(int argc, char** argv)
{
    int ran = 0;
    for (const auto& g : GROUPS)
        if (argc < 2 || std::string(argv[1]) == g.name) {
            g.run();
            ran++;
        }
    if (!ran) {
        std::fprintf(stderr, "no such group: %s\n", argv[1]);
        return 2;
    }
    std::printf("%d group(s): all checks met\n", ran);
    return 0;
}
