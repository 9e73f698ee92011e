// ptsched_main.cpp -- TEST HARNESS ONLY: the host-side decisions of the parallel-tempering samplers
// (carma_pack_amd/csrc/carma_pt_sched.h) as a stand-alone program without HIP and without Python: the form in which they can run
// under the host sanitizers (g++ -fsanitize=address,undefined).  tests/test_pt_sched_cpu.py builds and runs it plain.
// Usage: ptsched_main [group]; no argument runs every group.  Exit status 0: every check met; 1: the first miss, named on stderr.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "carma_pt_sched.h"

namespace {

#define CHECK(cond, ...)                                                           \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "MISS %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                     \
            std::fprintf(stderr, "\n");                                            \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

std::vector<long> chunks(long niter, long chunk0, int thin)
{
    std::vector<long> out;
    for (long left = niter; left > 0; left -= out.back()) {
        out.push_back(carma::pt_next_chunk(left, chunk0, thin));
        CHECK(out.back() > 0 && out.back() <= left, "niter %ld chunk0 %ld thin %d: chunk %ld of %ld left", niter, chunk0, thin, out.back(),
              left);
    }
    return out;
}

// the sequences of the three loops this function replaced, derived by hand from them
void chunk_sequences()
{
    CHECK((chunks(10, 4, 0) == std::vector<long>{4, 4, 2}), "(10, 4, 0)");
    CHECK((chunks(10, 4, 3) == std::vector<long>{3, 3, 3, 1}), "(10, 4, 3)");
    CHECK((chunks(12, 4, 5) == std::vector<long>{5, 5, 2}), "(12, 4, 5)");
    CHECK((chunks(8, 4, 2) == std::vector<long>{4, 4}), "(8, 4, 2)");
    CHECK((chunks(1, 4096, 1) == std::vector<long>{1}), "(1, 4096, 1)");
}

void chunk_properties()
{
    for (long niter = 0; niter <= 200; niter++)
        for (long chunk0 : {1L, 3L, 16L, 4096L})
            for (int thin : {0, 1, 2, 7}) {
                long sum = 0, saved = 0;
                for (long ch : chunks(niter, chunk0, thin)) {      // (positive: checked in chunks)
                    sum += ch;
                    if (thin > 0 && niter % thin == 0) {
                        CHECK(ch % thin == 0, "niter %ld chunk0 %ld thin %d: chunk %ld is no multiple of thin", niter, chunk0, thin, ch);
                        saved += ch / thin;                         // what *save_offset advances by
                    }
                }
                CHECK(sum == niter, "niter %ld chunk0 %ld thin %d: chunks sum to %ld", niter, chunk0, thin, sum);
                if (thin > 0 && niter % thin == 0) CHECK(saved == niter / thin, "niter %ld chunk0 %ld thin %d: %ld saved", niter, chunk0, thin, saved);
            }
}

void ladder()
{
    std::vector<double> t;
    carma::default_ladder(1, nullptr, t);
    CHECK(t.size() == 1 && t[0] == 1.0, "T = 1");
    carma::default_ladder(3, nullptr, t);
    CHECK(t.size() == 3 && t[0] == 1.0, "T = 3: first entry %.17g", t[0]);
    CHECK(std::fabs(t[1] / 10.0 - 1.0) <= 1e-14 && std::fabs(t[2] / 100.0 - 1.0) <= 1e-14, "T = 3: %.17g %.17g", t[1], t[2]);
    for (int T = 2; T <= 64; T++) {
        carma::default_ladder(T, nullptr, t);
        CHECK((int)t.size() == T && t[0] == 1.0, "T = %d", T);
        for (int i = 1; i < T; i++) CHECK(t[i] > t[i - 1], "T = %d: entry %d does not increase", T, i);
    }
    const double given[4] = {1.0, 2.5, 2.5, 0.3};                  // whatever the caller passes, as it is
    carma::default_ladder(4, given, t);
    CHECK(t.size() == 4 && std::memcmp(t.data(), given, sizeof given) == 0, "given temperatures changed");
}

void factor_var_rng()
{
    double R0[25];
    for (double& v : R0) v = -1.0;
    carma::initial_factor(2.0, 8, 5, R0);
    for (int i = 0; i < 5; i++)
        for (int j = 0; j < 5; j++) {
            const double want = i != j ? 0.0 : (i == 0 ? 1.0 : (i == 2 ? 0.5 : 0.01));
            CHECK(R0[i * 5 + j] == want, "initial_factor [%d][%d] = %.17g, expected %.17g", i, j, R0[i * 5 + j], want);
        }
    const double y[4] = {1, 2, 3, 4};
    CHECK(carma::pop_var(y, 4) == 1.25, "pop_var = %.17g", carma::pop_var(y, 4));
    // first outputs of the generator a chain's draws come from; std::mt19937_64 is fixed by the standard
    const struct { uint64_t seed, slot; int round; uint64_t first; } keys[4] = {{0, 0, 0, 7180524179296925545ull},
                                                                                {1, 0, 0, 11699722124793075009ull},
                                                                                {1, 7, 0, 1898596055538401877ull},
                                                                                {1, 7, 3, 8392547920658350700ull}};
    for (const auto& k : keys) {
        const uint64_t got = carma::start_rng(k.seed, k.slot, k.round)();
        CHECK(got == k.first, "start_rng(%llu, %llu, %d) gives %llu", (unsigned long long)k.seed, (unsigned long long)k.slot, k.round,
              (unsigned long long)got);
    }
}

// draw_start by its bounds only: its distributions are the C++ library's
void draws()
{
    const int n = 40;
    std::vector<double> t(n), y(n);
    uint64_t s = 99;
    auto uni = [&s] { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; };
    double now = 0;
    for (int i = 0; i < n; i++) {
        now += 0.05 + 3.0 * uni();
        t[i] = now;
        y[i] = 10.0 + uni() - uni();
    }
    const carma::Prior pr_series{7.0, 10.0, 1.0 / (10.0 * (t[n - 1] - t[0])), 50.0};
    const int cases[6][2] = {{1, 0}, {2, 1}, {3, 0}, {5, 3}, {6, 0}, {7, 6}};
    for (const auto& pq : cases) {
        const int p = pq[0], q = pq[1], d = p == 1 ? 4 : 3 + p + q;
        carma::Prior pr = pr_series;
        if (p == 1) pr.max_freq = -2.0;      // low enough to cut some of the draws of theta[3] = -log(median dt (1 ... 50)) (about -4.3 ... -0.4)
        for (uint64_t slot = 0; slot < 200; slot++) {
            std::vector<double> a(d), b(d);
            std::mt19937_64 r1 = carma::start_rng(5, slot, 0), r2 = carma::start_rng(5, slot, 0);
            carma::draw_start(t.data(), y.data(), n, pr, p, q, r1, a.data());
            carma::draw_start(t.data(), y.data(), n, pr, p, q, r2, b.data());
            CHECK(std::memcmp(a.data(), b.data(), sizeof(double) * d) == 0, "p %d q %d slot %d: the same key, another vector", p, q, (int)slot);
            CHECK(a[1] >= 0.51 && a[1] <= 1.99, "p %d q %d: theta[1] = %.17g", p, q, a[1]);
            CHECK(a[0] > 0, "p %d q %d: theta[0] = %.17g", p, q, a[0]);
            if (p == 1) CHECK(a[3] <= pr.max_freq, "p = 1: theta[3] = %.17g above max_freq", a[3]);
            for (int j = 0; j < d; j++) CHECK(std::isfinite(a[j]), "p %d q %d: theta[%d] = %g", p, q, j, a[j]);
        }
    }
}

// find_starts with fake callables: chain k becomes finite in round finite_at[k] (never: -1); candidates and values name their
// (chain, round)
void starts()
{
    const int d = 3;
    const double NEG = -std::numeric_limits<double>::infinity();
    const std::vector<int> finite_at = {0, 2, 0, -7 /* done on entry */, 5, 1, -7, 0};
    const size_t nchain = finite_at.size();
    std::vector<double> theta(nchain * d, -1.0), lp(nchain, NEG);
    std::vector<char> done(nchain, 0);
    for (size_t k = 0; k < nchain; k++)
        if (finite_at[k] == -7) {
            done[k] = 1;
            lp[k] = 123.0 + k;
            for (int j = 0; j < d; j++) theta[k * d + j] = 1000.0 * k + j;
        }
    long ndraw = 0, neval = 0;
    auto draw = [&](size_t k, int round, double* out) {
        CHECK(k < nchain && finite_at[k] != -7, "chain %zu was done on entry and is drawn for", k);
        CHECK(!done[k], "chain %zu is done and is drawn for in round %d", k, round);
        for (int j = 0; j < d; j++) out[j] = 100.0 * k + 10.0 * round + j;
        ndraw++;
    };
    auto evaluate = [&](const double* cand, const size_t* idx, size_t m, double* out) {
        for (size_t i = 0; i < m; i++) {
            const size_t k = idx[i];
            CHECK(k < nchain && !done[k], "evaluate sees chain %zu, which is done", k);
            CHECK(i == 0 || idx[i - 1] < k, "evaluate: chains out of order");
            const int round = (int)((cand[i * d] - 100.0 * k) / 10.0);
            CHECK(cand[i * d + 1] == 100.0 * k + 10.0 * round + 1, "evaluate: candidate %zu is not chain %zu's", i, k);
            out[i] = round >= finite_at[k] ? -(double)(1000 * k + round) : (round % 2 ? NEG : std::nan(""));
            neval++;
        }
        return 0;
    };
    int rc = carma::find_starts(nchain, d, theta.data(), lp.data(), done.data(), draw, evaluate);
    CHECK(rc == 0, "rc = %d", rc);
    long want = 0;
    for (size_t k = 0; k < nchain; k++) {
        CHECK(done[k], "chain %zu not done", k);
        if (finite_at[k] == -7) {
            CHECK(lp[k] == 123.0 + k && theta[k * d + 2] == 1000.0 * k + 2, "chain %zu was done on entry and has changed", k);
            continue;
        }
        const int r = finite_at[k];
        want += r + 1;
        CHECK(lp[k] == -(double)(1000 * k + r), "chain %zu: value %.17g is not round %d's", k, lp[k], r);
        for (int j = 0; j < d; j++) CHECK(theta[k * d + j] == 100.0 * k + 10.0 * r + j, "chain %zu: candidate is not round %d's", k, r);
    }
    CHECK(ndraw == want && neval == want, "%ld draws, %ld evaluations, expected %ld each", ndraw, neval, want);

    // never finite: pending after exactly START_ROUNDS rounds; its neighbour is settled in round 0 and left alone afterwards
    std::vector<double> th2(2 * d, -1.0), lp2(2, NEG);
    std::vector<char> done2(2, 0);
    long rounds = 0, seen1 = 0;
    rc = carma::find_starts(
        2, d, th2.data(), lp2.data(), done2.data(), [&](size_t k, int round, double* out) { out[0] = out[1] = out[2] = (double)(k + round); },
        [&](const double*, const size_t* idx, size_t m, double* out) {
            rounds++;
            for (size_t i = 0; i < m; i++) {
                seen1 += idx[i] == 1;
                out[i] = idx[i] == 1 ? 4.0 : NEG;
            }
            return 0;
        });
    CHECK(carma::START_ROUNDS == 4000, "START_ROUNDS = %d", carma::START_ROUNDS);
    CHECK(rc == 0 && rounds == 4000 && seen1 == 1, "rc %d after %ld rounds, chain 1 evaluated %ld times", rc, rounds, seen1);
    CHECK(!done2[0] && done2[1] && lp2[0] == NEG && lp2[1] == 4.0 && th2[0] == -1.0, "the chain that is never finite was touched");

    // an error code of evaluate comes back at once
    std::vector<char> done3(2, 0);
    rounds = 0;
    rc = carma::find_starts(
        2, d, th2.data(), lp2.data(), done3.data(), [&](size_t, int, double* out) { out[0] = out[1] = out[2] = 0.0; },
        [&](const double*, const size_t*, size_t m, double* out) {
            std::fill(out, out + m, NEG);
            return ++rounds == 3 ? -22 : 0;
        });
    CHECK(rc == -22 && rounds == 3, "rc %d after %ld rounds", rc, rounds);
    CHECK(!done3[0] && !done3[1], "a chain was marked done without a finite value");
}

const struct { const char* name; void (*run)(); } GROUPS[] = {{"chunk_sequences", chunk_sequences}, {"chunk_properties", chunk_properties},
                                                               {"ladder", ladder},           {"factor_var_rng", factor_var_rng},
                                                               {"draws", draws},             {"starts", starts}};

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
