// hostmath.cpp -- TEST HARNESS ONLY: the HOST build of carma_math.h behind the same entry as devprim.hip's devprim_math
// (tests/test_devprim_cpu.py: the inputs and bounds of the device tests can be met by a correct implementation, and the
// host-side error maxima the device bounds refer to).
#include <cmath>
#define CARMA_DEV static inline
#include "carma_math.h"
using namespace carma;

extern "C" int hostmath(int fn, int n, const double* a, const double* b, const double* dt, const double* dt_lo, double* o0, double* o1)
{
    for (int i = 0; i < n; i++) {
        double r0 = 0.0, r1 = 0.0;
        switch (fn) {
            case 0: r0 = exp_neg(a[i]); break;
            case 1: r0 = exp_neg_tab(a[i], h_math_tab); break;
            case 2: sincos_cw(a[i], &r0, &r1); break;
            case 3: cexp_step<false>(a[i], b[i], dt[i], &r0, &r1); break;
            case 4: cexp_step_tab<false>(a[i], b[i], dt[i], &r0, &r1, h_math_tab); break;
            case 5: cexp_step<true>(a[i], b[i], dt[i], &r0, &r1, dt_lo[i]); break;
            case 6: cexp_step_tab<true>(a[i], b[i], dt[i], &r0, &r1, h_math_tab); break;
            default: return 1;
        }
        o0[i] = r0;
        o1[i] = r1;
    }
    return 0;
}
