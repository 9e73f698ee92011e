// hostmem_main.cpp -- TEST HARNESS ONLY: the device-buffer owner (carma_pack_amd/csrc/carma_devbuf.h) and the model-row packers
// (carma_model_pack.h) of the host layer as a stand-alone program without the HIP runtime and without Python: the form in which
// they can run under the host sanitizers (g++ -fsanitize=address,undefined).  tests/test_hostmem_cpu.py builds and runs it plain.
// carma_dev_malloc / carma_dev_free are defined HERE, over malloc / free: they record every request and every release, and can
// be told to fail the k-th request.
// Usage: hostmem_main [group]; no argument runs every group.  Exit status 0: every check met; 1: the first miss, named on stderr.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "carma_devbuf.h"
#include "carma_model_pack.h"

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
    char kind;                  // 'M': a request (n = its size; p = null when it was failed), 'F': a release
    size_t n;
    void* p;
};
std::vector<Event> g_log;
std::map<void*, size_t> g_live;
long g_fail_in = 0;             // > 0: the g_fail_in-th request from now fails
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
size_t frees()
{
    size_t k = 0;
    for (const Event& e : g_log) k += e.kind == 'F';
    return k;
}
}  // namespace

hipError_t carma_dev_malloc(void** p, size_t n)
{
    if (g_fail_in > 0 && --g_fail_in == 0) {
        g_log.push_back({'M', n, nullptr});
        *p = &g_poison;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(n ? n : 1);
    CHECK(*p, "malloc(%zu)", n);
    g_live[*p] = n;
    g_log.push_back({'M', n, *p});
    return hipSuccess;
}
hipError_t carma_dev_free(void* p)
{
    CHECK(p, "release of a null pointer reached the allocator");
    CHECK(g_live.count(p) == 1, "release of %p, which is not live (released twice, or never allocated)", p);
    g_live.erase(p);
    g_log.push_back({'F', 0, p});
    std::free(p);
    return hipSuccess;
}

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

const struct { const char* name; void (*run)(); } GROUPS[] = {{"devmem_alloc", devmem_alloc}, {"devmem_need", devmem_need}, {"roots", roots}, {"rows", rows}};

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
