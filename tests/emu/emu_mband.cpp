// emu_mband.cpp -- builds carma_pack_amd/csrc/carma_mband.h for the host.
// TEST HARNESS ONLY (see grp_emu.h): the multi-band lane filter exactly as the gfx950 kernel compiles it, one evaluation at a
// time, the records from the library's own packer (mband_pack).
#include <vector>
#include "grp_emu.h"
#include "../../carma_pack_amd/csrc/carma_core.h"
#include "../../carma_pack_amd/csrc/carma_lane.h"
#include "../../carma_pack_amd/csrc/carma_mband.h"

using namespace carma;

template <int P>
static double one(const double* thx, int q, int K, int N, const double4* rec, const int* boff, const double* lagbox, const Prior& pr,
                  int ignore_prior)
{
    const size_t KL = (size_t)K * MBAND_LANES;
    std::vector<double> w(5 * KL, 0.0);
    std::vector<int> pos(KL, 0);
    MbandWork wk{w.data(), w.data() + KL, w.data() + 2 * KL, w.data() + 3 * KL, w.data() + 4 * KL, pos.data(), boff};
    return logdensity_mband_lane<P>(thx, q, K, N, rec, lagbox, pr, ignore_prior, h_math_tab, wk);
}

// time / y / yerr: the bands one after another, each sorted and without duplicate times; offsets = [K + 1]; thx = [B][dx];
// lagbox = [K - 1][2]; prior = max_stdev, max_freq, min_freq, measerr_dof
extern "C" int emu_mband_logdensity(int p, int q, int K, const double* time, const double* y, const double* yerr, const long* offsets,
                                    const double* thx, int B, const double* lagbox, const double* prior, int ignore_prior,
                                    double* out)
{
    if (K < 1 || K > MBAND_KMAX) return -1;
    std::vector<std::vector<double>> ts(K), ys(K), es(K);
    for (int b = 0; b < K; b++) {
        ts[b].assign(time + offsets[b], time + offsets[b + 1]);
        ys[b].assign(y + offsets[b], y + offsets[b + 1]);
        es[b].assign(yerr + offsets[b], yerr + offsets[b + 1]);
    }
    std::vector<double> rec;
    std::vector<int> boff;
    mband_pack(ts, ys, es, rec, boff);
    const double4* r4 = reinterpret_cast<const double4*>(rec.data());
    const int N = (int)offsets[K], dx = 3 + p + q + 3 * (K - 1);
    const Prior pr{prior[0], prior[1], prior[2], prior[3]};
    for (int i = 0; i < B; i++) {
        const double* th = thx + (size_t)i * dx;
        switch (p) {
            case 1: out[i] = one<1>(th, q, K, N, r4, boff.data(), lagbox, pr, ignore_prior); break;
            case 2: out[i] = one<2>(th, q, K, N, r4, boff.data(), lagbox, pr, ignore_prior); break;
            case 3: out[i] = one<3>(th, q, K, N, r4, boff.data(), lagbox, pr, ignore_prior); break;
            case 4: out[i] = one<4>(th, q, K, N, r4, boff.data(), lagbox, pr, ignore_prior); break;
            case 5: out[i] = one<5>(th, q, K, N, r4, boff.data(), lagbox, pr, ignore_prior); break;
            case 6: out[i] = one<6>(th, q, K, N, r4, boff.data(), lagbox, pr, ignore_prior); break;
            case 7: out[i] = one<7>(th, q, K, N, r4, boff.data(), lagbox, pr, ignore_prior); break;
            default: return -1;
        }
    }
    return 0;
}
