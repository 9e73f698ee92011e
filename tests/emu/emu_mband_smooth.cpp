// emu_mband_smooth.cpp -- builds carma_pack_amd/csrc/carma_mband_smooth.h for the host.
// TEST HARNESS ONLY (see grp_emu.h): the two passes of the multi-band smoother exactly as the gfx950 kernels compile them, one
// parameter vector at a time, the records from the library's own packer (mband_pack) and planner (mband_smooth_times).
#include <algorithm>
#include <vector>
#include "grp_emu.h"
#include "../../carma_pack_amd/csrc/carma_core.h"
#include "../../carma_pack_amd/csrc/carma_lane.h"
#include "../../carma_pack_amd/csrc/carma_mband.h"
#include "../../carma_pack_amd/csrc/carma_mband_smooth.h"
#include "../../carma_pack_amd/csrc/carma_mband_smooth_plan.h"

using namespace carma;

template <int P>
static int one(const double* thx, int q, int K, int N, int M, int bo, const double4* rec, const int* boff, const double4* req,
               double* mean, double* var)
{
    static_assert(mband_smooth_fields<P>() == mband_smooth_nfields(P), "header and planner disagree on the record");
    const size_t KL = (size_t)(K + 1) * MBAND_LANES;
    std::vector<double> w(5 * KL, 0.0);
    std::vector<int> pos(KL, 0);
    MbandWork wk{w.data(), w.data() + KL, w.data() + 2 * KL, w.data() + 3 * KL, w.data() + 4 * KL, pos.data(), boff};
    MbandSmoothLane<P> s;
    mband_smooth_setup<P>(thx, q, K, bo, s, &wk);
    bool anyreal = false;
    for (int i = 0; i < P / 2; i++) anyreal = anyreal || s.m.realpair[i];
    // one lane of the device layout [point][field][64]
    const MbandSmoothStrides sd = mband_smooth_strides(P, N + M);
    std::vector<double> sc(sd.ws, 0.0);
    lane_smooth_forward_mband<P>(s.m, anyreal, h_math_tab, rec, req, K, N, M, wk, sc.data() + 17, sd.fs, sd.ps);
    // the backward pass from a setup of its own, as the second kernel makes it
    MbandSmoothLane<P> s2;
    mband_smooth_setup<P>(thx, q, K, bo, s2, nullptr);
    lane_smooth_backward_mband<P>(s2.m, s2.a_o, s2.mu_o, !s2.ok, N + M, sc.data() + 17, sd.fs, sd.ps, M, mean, var);
    return s2.ok ? 0 : 1;
}

// time / y / yerr: the bands one after another, each sorted and without duplicate times; offsets = [K + 1]; thx = [B][dx];
// tout = [M] in any order; mean / var = [B][M]; invalid = [B]
extern "C" int emu_mband_smooth(int p, int q, int K, const double* time, const double* y, const double* yerr, const long* offsets,
                                const double* thx, int B, int band, const double* tout, int M, double* mean, double* var,
                                int* invalid)
{
    if (K < 1 || K > MBAND_KMAX || band < 0 || band >= K || M < 1) return -1;
    std::vector<std::vector<double>> ts(K), ys(K), es(K);
    double t0 = time[0];
    for (int b = 0; b < K; b++) {
        ts[b].assign(time + offsets[b], time + offsets[b + 1]);
        ys[b].assign(y + offsets[b], y + offsets[b + 1]);
        es[b].assign(yerr + offsets[b], yerr + offsets[b + 1]);
        t0 = std::min(t0, ts[b][0]);
    }
    std::vector<double> rec;
    std::vector<int> boff;
    mband_pack(ts, ys, es, rec, boff);
    const MbandSmoothTimes tm = mband_smooth_times(tout, M, t0);
    const double4* r4 = reinterpret_cast<const double4*>(rec.data());
    const double4* q4 = reinterpret_cast<const double4*>(tm.rec.data());
    const int N = (int)offsets[K], dx = 3 + p + q + 3 * (K - 1);
    for (int i = 0; i < B; i++) {
        const double* th = thx + (size_t)i * dx;
        double *pm = mean + (size_t)i * M, *pv = var + (size_t)i * M;
        switch (p) {
            case 1: invalid[i] = one<1>(th, q, K, N, M, band, r4, boff.data(), q4, pm, pv); break;
            case 2: invalid[i] = one<2>(th, q, K, N, M, band, r4, boff.data(), q4, pm, pv); break;
            case 3: invalid[i] = one<3>(th, q, K, N, M, band, r4, boff.data(), q4, pm, pv); break;
            case 4: invalid[i] = one<4>(th, q, K, N, M, band, r4, boff.data(), q4, pm, pv); break;
            case 5: invalid[i] = one<5>(th, q, K, N, M, band, r4, boff.data(), q4, pm, pv); break;
            case 6: invalid[i] = one<6>(th, q, K, N, M, band, r4, boff.data(), q4, pm, pv); break;
            case 7: invalid[i] = one<7>(th, q, K, N, M, band, r4, boff.data(), q4, pm, pv); break;
            default: return -1;
        }
    }
    return 0;
}
