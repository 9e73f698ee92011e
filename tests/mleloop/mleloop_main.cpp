// mleloop_main.cpp -- TEST HARNESS ONLY: the library's lock-step loop (carma_pack_amd/csrc/carma_mle_loop.h) on objectives with
// known answers, as a stand-alone program without Python: the form in which the loop's index arithmetic can run under the
// host sanitizers (g++ -fsanitize=address,undefined).  tests/test_mle_loop_cpu.py builds and runs it plain.  Exit status 0: every
// case met; 1: a miss, named on stderr.
//
// Cases: box-constrained convex quadratics against an enumeration of the active sets; every start its own separable problem in
// its own box (answer clip(c, lo, hi)); the kink on which no step length is accepted; short memories (drop-oldest path).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "carma_mle_loop.h"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            g_fail++;                             \
            std::fprintf(stderr, "MISS %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);    \
            std::fprintf(stderr, "\n");           \
        }                                         \
    } while (0)

struct Lcg {                                      // a small generator of its own: the cases are the same everywhere
    uint64_t s;
    double uni() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0; }
    double uni(double a, double b) { return a + (b - a) * uni(); }
};

const double INF = std::numeric_limits<double>::infinity();
const double GTOL = 1e-5, FD = 1e-6;

// f = 1/2 (x - c)' H (x - c)
struct Quad {
    static constexpr bool PER_START = false;
    int d;
    std::vector<double> H, c;
    std::vector<double> out;
    double fmax = 0.0;
    double value(const double* x) const
    {
        double s = 0.0;
        for (int i = 0; i < d; i++) {
            double r = 0.0;
            for (int j = 0; j < d; j++) r += H[(size_t)i * d + j] * (x[j] - c[j]);
            s += (x[i] - c[i]) * r;
        }
        return 0.5 * s;
    }
    int operator()(const std::vector<double>& pts, const std::vector<int>&, int npts)
    {
        out.resize((size_t)npts);
        for (int k = 0; k < npts; k++) {
            out[k] = value(&pts[(size_t)k * d]);
            fmax = std::max(fmax, std::fabs(out[k]));
        }
        return CARMA_OK;
    }
};

// H = Q diag(lam) Q', Q a Householder reflection, lam geometric from 1 to cond
Quad make_quad(int d, double cond, Lcg& rng)
{
    Quad q;
    q.d = d;
    q.H.assign((size_t)d * d, 0.0);
    q.c.resize(d);
    std::vector<double> v(d), lam(d), Q((size_t)d * d);
    double vv = 0.0;
    for (int i = 0; i < d; i++) {
        v[i] = rng.uni(-1.0, 1.0);
        vv += v[i] * v[i];
        lam[i] = d == 1 ? 1.0 : std::pow(cond, (double)i / (d - 1));
        q.c[i] = rng.uni(-2.0, 2.0);
    }
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) Q[(size_t)i * d + j] = (i == j ? 1.0 : 0.0) - 2.0 * v[i] * v[j] / vv;
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++)
            for (int k = 0; k < d; k++) q.H[(size_t)i * d + j] += Q[(size_t)i * d + k] * lam[k] * Q[(size_t)j * d + k];
    return q;
}

// Gaussian elimination with partial pivoting; returns false when singular
bool solve(std::vector<double> A, std::vector<double> b, int n, std::vector<double>& x)
{
    for (int k = 0; k < n; k++) {
        int p = k;
        for (int i = k + 1; i < n; i++)
            if (std::fabs(A[(size_t)i * n + k]) > std::fabs(A[(size_t)p * n + k])) p = i;
        if (std::fabs(A[(size_t)p * n + k]) < 1e-300) return false;
        for (int j = 0; j < n; j++) std::swap(A[(size_t)k * n + j], A[(size_t)p * n + j]);
        std::swap(b[k], b[p]);
        for (int i = k + 1; i < n; i++) {
            const double m = A[(size_t)i * n + k] / A[(size_t)k * n + k];
            for (int j = k; j < n; j++) A[(size_t)i * n + j] -= m * A[(size_t)k * n + j];
            b[i] -= m * b[k];
        }
    }
    x.assign(n, 0.0);
    for (int i = n - 1; i >= 0; i--) {
        double s = b[i];
        for (int j = i + 1; j < n; j++) s -= A[(size_t)i * n + j] * x[j];
        x[i] = s / A[(size_t)i * n + i];
    }
    return true;
}

// The minimiser over [-1, 1]^d by enumeration of the 3^d active sets: each variable at -1, at +1 or free; the free ones solve
// their linear system; the candidate that is feasible and has multipliers of the right sign is the answer (strictly convex:
// unique).  state[j]: -1 / +1 at that bound, 0 free.
bool active_set_answer(const Quad& q, std::vector<double>& xs, std::vector<int>& state)
{
    const int d = q.d;
    int total = 1;
    for (int j = 0; j < d; j++) total *= 3;
    for (int code = 0; code < total; code++) {
        std::vector<int> st(d);
        std::vector<int> fr;
        int cc = code;
        for (int j = 0; j < d; j++, cc /= 3) {
            st[j] = cc % 3 - 1;
            if (st[j] == 0) fr.push_back(j);
        }
        std::vector<double> x(d);
        for (int j = 0; j < d; j++) x[j] = (double)st[j];
        const int nf = (int)fr.size();
        if (nf) {                                  // H_ff (x_f - c_f) = -H_fb (x_b - c_b)
            std::vector<double> A((size_t)nf * nf), b(nf), y;
            for (int a = 0; a < nf; a++) {
                b[a] = 0.0;
                for (int e = 0; e < nf; e++) A[(size_t)a * nf + e] = q.H[(size_t)fr[a] * d + fr[e]];
                for (int j = 0; j < d; j++)
                    if (st[j] != 0) b[a] -= q.H[(size_t)fr[a] * d + j] * (x[j] - q.c[j]);
            }
            if (!solve(A, b, nf, y)) continue;
            for (int a = 0; a < nf; a++) x[fr[a]] = q.c[fr[a]] + y[a];
        }
        bool ok = true;
        for (int j = 0; j < d && ok; j++) {
            double gj = 0.0;
            for (int k = 0; k < d; k++) gj += q.H[(size_t)j * d + k] * (x[k] - q.c[k]);
            if (st[j] == 0) ok = x[j] > -1.0 && x[j] < 1.0;
            else ok = st[j] < 0 ? gj > 0.0 : gj < 0.0;
        }
        if (ok) {
            xs = x;
            state = st;
            return true;
        }
    }
    return false;
}

// ||x - x*|| on the free variables <= sqrt(d) (gtol + delta) / lam_min: every free component of the difference quotient is
// within gtol, the quotient of a quadratic is its gradient up to the rounding delta = 4 eps max|f| / (2 fd_step max(1, |x|)) of
// the two values it subtracts (the coordinate with the smallest step decides), and ||x - x*|| <= ||g|| / lam_min.
double answer_bound(int d, double fmax, double lam_min, const double* x)
{
    double xs = INF;
    for (int j = 0; j < d; j++) xs = std::min(xs, std::max(1.0, std::fabs(x[j])));
    return std::sqrt((double)d) * (GTOL + 4.0 * DBL_EPSILON * fmax / (2.0 * FD * xs)) / lam_min;
}

void case_quadratic(int d, double cond, int mem, int B, uint64_t seed)
{
    Lcg rng{seed};
    Quad q = make_quad(d, cond, rng);
    std::vector<double> xs;
    std::vector<int> st;
    if (!active_set_answer(q, xs, st)) {
        CHECK(false, "no active set found (d %d cond %g)", d, cond);
        return;
    }
    std::vector<double> x0((size_t)B * d), lo(d, -1.0), hi(d, 1.0), x((size_t)B * d), f(B);
    for (auto& v : x0) v = rng.uni(-1.5, 1.5);      // some outside the box: projected first
    std::vector<int> nit(B), nfev(B), status(B);
    const int rc = carma::mle_loop(q, d, x0.data(), B, lo.data(), hi.data(), 0, 2000, mem, 0.0, GTOL, FD, x.data(), f.data(),
                                   nit.data(), nfev.data(), status.data());
    CHECK(rc == CARMA_OK, "rc %d", rc);
    int nitmax = 0;
    double bound = 0.0;
    for (int b = 0; b < B; b++) {
        bound = answer_bound(d, q.fmax, 1.0, &x[(size_t)b * d]);
        CHECK(status[b] == 0, "quadratic d %d cond %g mem %d start %d: status %d nit %d", d, cond, mem, b, status[b], nit[b]);
        double e2 = 0.0;
        for (int j = 0; j < d; j++) {
            const double xv = x[(size_t)b * d + j];
            if (st[j] != 0) CHECK(xv == (double)st[j], "start %d coordinate %d: %.17g is not on its bound %d", b, j, xv, st[j]);
            else e2 += (xv - xs[j]) * (xv - xs[j]);
        }
        CHECK(std::sqrt(e2) <= bound, "quadratic d %d cond %g mem %d start %d: %.3e from the answer, bound %.3e", d, cond, mem, b,
              std::sqrt(e2), bound);
        CHECK(f[b] == q.value(&x[(size_t)b * d]), "start %d: fun is not f(x)", b);
        nitmax = std::max(nitmax, nit[b]);
    }
    if (mem <= 2 && d >= 3 && cond > 1.0) CHECK(nitmax > mem + 1, "memory case d %d mem %d never filled its history (nit <= %d)", d, mem, nitmax);
    std::printf("quadratic d=%d cond=%g mem=%d B=%d: nit <= %d, bound %.2e\n", d, cond, mem, B, nitmax, bound);
}

// start b minimises sum_j w_bj (x_j - c_bj)^2 in its own box
struct Sep {
    static constexpr bool PER_START = true;
    int d;
    std::vector<double> w, c, lo, hi;
    std::vector<double> out;
    std::vector<double> fmax;
    int outside = 0, badowner = 0;
    int B;
    int operator()(const std::vector<double>& pts, const std::vector<int>& owner, int npts)
    {
        out.resize((size_t)npts);
        for (int k = 0; k < npts; k++) {
            const int b = owner[k];
            if (b < 0 || b >= B) {
                badowner++;
                out[k] = 0.0;
                continue;
            }
            double s = 0.0;
            for (int j = 0; j < d; j++) {
                const double xv = pts[(size_t)k * d + j];
                if (xv < lo[(size_t)b * d + j] || xv > hi[(size_t)b * d + j]) outside++;
                s += w[(size_t)b * d + j] * (xv - c[(size_t)b * d + j]) * (xv - c[(size_t)b * d + j]);
            }
            out[k] = s;
            fmax[b] = std::max(fmax[b], s);
        }
        return CARMA_OK;
    }
};

void case_clip(int B, uint64_t seed)
{
    const int d = 3;
    Lcg rng{seed};
    Sep p;
    p.d = d;
    p.B = B;
    p.w.resize((size_t)B * d);
    p.c.resize((size_t)B * d);
    p.lo.resize((size_t)B * d);
    p.hi.resize((size_t)B * d);
    p.fmax.assign(B, 0.0);
    std::vector<double> x0((size_t)B * d), x((size_t)B * d), f(B);
    for (int b = 0; b < B; b++) {
        const double scale = std::pow(10.0, rng.uni(-2.0, 2.0));
        for (int j = 0; j < d; j++) {
            const size_t k = (size_t)b * d + j;
            p.w[k] = scale * rng.uni(1.0, 4.0);
            p.c[k] = rng.uni(-2.0, 2.0) + b;
            p.lo[k] = b + rng.uni(-1.5, 0.0);
            p.hi[k] = b + rng.uni(0.0, 1.5);
            x0[k] = b + rng.uni(-2.0, 2.0);
        }
        const size_t k0 = (size_t)b * d;
        switch (b % 5) {
            case 0: p.hi[k0 + b % d] = p.lo[k0 + b % d]; break;              // lo = hi in one coordinate
            case 1: p.lo[k0 + (b + 1) % d] = -INF; break;                    // one-sided
            case 2: p.hi[k0 + (b + 2) % d] = INF; break;
            case 3: for (int j = 0; j < d; j++) p.lo[k0 + j] = -INF, p.hi[k0 + j] = INF; break;   // wholly infinite
            default: break;
        }
    }
    std::vector<int> nit(B), nfev(B), status(B);
    const int rc = carma::mle_loop(p, d, x0.data(), B, p.lo.data(), p.hi.data(), (size_t)d, 2000, 8, 0.0, GTOL, FD, x.data(), f.data(),
                                   nit.data(), nfev.data(), status.data());
    CHECK(rc == CARMA_OK, "rc %d", rc);
    CHECK(p.outside == 0, "clip B %d: %d coordinates evaluated outside their owner's box", B, p.outside);
    CHECK(p.badowner == 0, "clip B %d: %d owners out of range", B, p.badowner);
    int nitmin = 1 << 30, nitmax = 0;
    for (int b = 0; b < B; b++) {
        CHECK(status[b] == 0, "clip B %d start %d: status %d", B, b, status[b]);
        double lam = INF, e2 = 0.0;
        for (int j = 0; j < d; j++) lam = std::min(lam, 2.0 * p.w[(size_t)b * d + j]);
        for (int j = 0; j < d; j++) {
            const size_t k = (size_t)b * d + j;
            const double want = std::min(std::max(p.c[k], p.lo[k]), p.hi[k]);
            if (p.lo[k] == p.hi[k]) CHECK(x[k] == p.lo[k], "clip start %d: pinned coordinate %d moved", b, j);
            if (want == p.lo[k] || want == p.hi[k]) CHECK(x[k] == want, "clip start %d coordinate %d: %.17g, bound %.17g", b, j, x[k], want);
            else e2 += (x[k] - want) * (x[k] - want);
        }
        const double bound = answer_bound(d, p.fmax[b], lam, &x[(size_t)b * d]);
        CHECK(std::sqrt(e2) <= bound, "clip B %d start %d: %.3e from the answer, bound %.3e", B, b, std::sqrt(e2), bound);
        nitmin = std::min(nitmin, nit[b]);
        nitmax = std::max(nitmax, nit[b]);
    }
    std::printf("clip B=%d: nit %d ... %d\n", B, nitmin, nitmax);
}

// f = sum |x - x0| + (x - x0)_0 / 2: the central difference says downhill along coordinate 0, but no step is
struct Kink {
    static constexpr bool PER_START = false;
    int d;
    std::vector<double> x0;
    std::vector<double> out;
    int operator()(const std::vector<double>& pts, const std::vector<int>&, int npts)
    {
        out.resize((size_t)npts);
        for (int k = 0; k < npts; k++) {
            double s = 0.5 * (pts[(size_t)k * d] - x0[0]);
            for (int j = 0; j < d; j++) s += std::fabs(pts[(size_t)k * d + j] - x0[j]);
            out[k] = s;
        }
        return CARMA_OK;
    }
};

void case_kink()
{
    const int d = 3;
    Kink k;
    k.d = d;
    k.x0 = {0.3, -0.7, 1.1};
    std::vector<double> lo(d, -INF), hi(d, INF), x(d), f(1);
    int nit, nfev, status;
    const int rc = carma::mle_loop(k, d, k.x0.data(), 1, lo.data(), hi.data(), 0, 50, 8, 0.0, GTOL, FD, x.data(), f.data(), &nit, &nfev,
                                   &status);
    CHECK(rc == CARMA_OK, "rc %d", rc);
    CHECK(status == 3 && nit == 0, "kink: status %d nit %d", status, nit);
    CHECK(nfev == 2 * d + 1 + 32, "kink: nfev %d", nfev);
    for (int j = 0; j < d; j++) CHECK(x[j] == k.x0[j], "kink: x moved");
    std::printf("kink: status %d nfev %d\n", status, nfev);
}

}  // namespace

int main()
{
    for (int d : {1, 3, 5})
        for (double cond : {1.0, 100.0}) case_quadratic(d, cond, 8, 20, 1000 + 10 * d + (cond > 1.0));
    for (int B : {1, 18, 19, 52, 60}) case_clip(B, 77 + B);
    case_kink();
    for (int mem : {1, 2, 64}) case_quadratic(5, 100.0, mem, 20, 4242);
    if (g_fail) {
        std::fprintf(stderr, "mleloop_main: %d misses\n", g_fail);
        return 1;
    }
    std::printf("mleloop_main: all cases met\n");
    return 0;
}
