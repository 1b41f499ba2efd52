// C shim over tools/sim3opt_ref.hpp for the Python checkers (tests/sim3opt_cases.py; built by tests/ref_shim.py).
#include "../../tools/sim3opt_ref.hpp"

using namespace sim3opt_ref;

extern "C" {

int sim3optref_sizes(int i) { return i == 0 ? (int)sizeof(Problem) : i == 1 ? (int)sizeof(Corr) : (int)sizeof(Result); }

// OptimizeSim3 of n_problems problems, problem p's correspondences being corrs[corr_start[p] .. corr_start[p + 1]).  mode 0:
// Serial, 1: Defined, 2: Defined with the 14 perturbed estimates taken once per linearisation (the device's evaluation).
// last_rejected (2 ints a problem) and class_chi2 (2 passes x 2 n doubles a problem, at 4 * corr_start[p]) may be null.
void sim3optref_run(int mode, const Problem* problems, int n_problems, const int32_t* corr_start, const Corr* corrs, Result* out, uint8_t* removed,
                    int32_t* last_rejected, double* class_chi2)
{
    for (int p = 0; p < n_problems; p++) {
        const int c0 = corr_start[p], n = corr_start[p + 1] - c0;
        Diag d;
        d.classChi2 = class_chi2 ? class_chi2 + (size_t)4 * c0 : nullptr;
        if (mode == 0) optimizeSim3<Serial>(problems[p], corrs + c0, n, out[p], removed + c0, &d, false);
        else optimizeSim3<Defined>(problems[p], corrs + c0, n, out[p], removed + c0, &d, mode == 2);
        if (last_rejected) for (int r = 0; r < 2; r++) last_rejected[p * 2 + r] = d.lastTrialRejected[r];
    }
}

void sim3optref_exp(const double* x, int n, double* e)
{
    for (int i = 0; i < n; i++) e[i] = definedExp(x[i]);
}

// Quaterniond(R), R row-major: for the mirror's sim3_from_rts
void sim3optref_quat(const double* R, double* q) { poseopt_ref::quatFromMatrix(R, q); }

static double ulpOf(double v)
{
    v = std::fabs(v);
    if (v < DBL_MIN) return DBL_MIN * DBL_EPSILON;
    int e;
    std::frexp(v, &e);
    return std::ldexp(1.0, e - 53);
}

// definedExp against libm over count arguments evenly spaced in [lo, hi]: the largest |defined - libm| in units of libm's
// value's last place, and the argument where it occurs
void sim3optref_exp_sweep(double lo, double hi, int64_t count, double* max_ulp, double* at)
{
    max_ulp[0] = 0.0;
    at[0] = lo;
    const double step = count > 1 ? (hi - lo) / (double)(count - 1) : 0.0;
    for (int64_t i = 0; i < count; i++) {
        volatile double x = lo + step * (double)i;
        const double e = definedExp(x), r = std::exp(x);
        const double err = std::fabs(e - r) / ulpOf(r);
        if (err > max_ulp[0]) { max_ulp[0] = err; at[0] = x; }
    }
}

}  // extern "C"
