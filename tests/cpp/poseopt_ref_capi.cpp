// C shim over tools/poseopt_ref.hpp for the Python checkers (tests/poseopt_cases.py; built by tests/ref_shim.py).
#include "../../tools/poseopt_ref.hpp"

using namespace poseopt_ref;

extern "C" {

int poseoptref_sizes(int i) { return i == 0 ? (int)sizeof(Frame) : i == 1 ? (int)sizeof(Edge) : (int)sizeof(Result); }

// PoseOptimization of n_frames frames, frame f's edges being edges[edge_start[f] .. edge_start[f + 1]).  mode 0: Serial,
// 1: Defined.  last_rejected (4 ints a frame) and class_chi2 (4 * n doubles a frame, at 4 * edge_start[f]) may be null.
void poseoptref_run(int mode, const Frame* frames, int n_frames, const int32_t* edge_start, const Edge* edges, Result* out, uint8_t* outlier,
                    int32_t* last_rejected, double* class_chi2)
{
    for (int f = 0; f < n_frames; f++) {
        const int e0 = edge_start[f], n = edge_start[f + 1] - e0;
        Diag d;
        d.classChi2 = class_chi2 ? class_chi2 + (size_t)4 * e0 : nullptr;
        if (mode == 0) poseOptimization<Serial>(frames[f], edges + e0, n, out[f], outlier + e0, &d);
        else poseOptimization<Defined>(frames[f], edges + e0, n, out[f], outlier + e0, &d);
        if (last_rejected) for (int r = 0; r < 4; r++) last_rejected[f * 4 + r] = d.lastTrialRejected[r];
    }
}

void poseoptref_sincos(const double* x, int n, double* s, double* c)
{
    for (int i = 0; i < n; i++) definedSinCos(x[i], s[i], c[i]);
}

static double ulpOf(double v)
{
    v = std::fabs(v);
    if (v < DBL_MIN) return DBL_MIN * DBL_EPSILON;
    int e;
    std::frexp(v, &e);
    return std::ldexp(1.0, e - 53);
}

// the Defined routine against libm over count arguments evenly spaced in [lo, hi]: the largest |defined - libm| in units of
// libm's value's last place, for sin and for cos, and the arguments where they occur
void poseoptref_sincos_sweep(double lo, double hi, int64_t count, double* max_ulp, double* at)
{
    max_ulp[0] = max_ulp[1] = 0.0;
    at[0] = at[1] = lo;
    const double step = count > 1 ? (hi - lo) / (double)(count - 1) : 0.0;
    for (int64_t i = 0; i < count; i++) {
        volatile double x = lo + step * (double)i;
        double s, c;
        definedSinCos(x, s, c);
        const double rs = std::sin(x), rc = std::cos(x);
        const double es = std::fabs(s - rs) / ulpOf(rs), ec = std::fabs(c - rc) / ulpOf(rc);
        if (es > max_ulp[0]) { max_ulp[0] = es; at[0] = x; }
        if (ec > max_ulp[1]) { max_ulp[1] = ec; at[1] = x; }
    }
}

}  // extern "C"
