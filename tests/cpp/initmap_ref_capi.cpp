// C shim over tools/initmap_ref.hpp for the Python checkers (tests/initmap_cases.py; built by tests/ref_shim.py).
#include "../../tools/initmap_ref.hpp"

using namespace initmap_ref;

extern "C" {

int initmapref_sizes(int i)
{
    return i == 0 ? (int)sizeof(Problem) : i == 1 ? (int)sizeof(Result) : i == 2 ? (int)sizeof(Point) : i == 3 ? (int)sizeof(Key) : (int)sizeof(Diag);
}

// one problem.  mode 0: Serial, 1: Defined.  diag may be null
void initmapref_run(int mode, const Problem* pr, const Key* keys1, const Key* keys2, const int32_t* matches12, const float* P3D,
                    const float* inv_level_sigma2, const float* scale_factors, int nlevels, Result* out, Point* points, Diag* diag)
{
    if (mode == 0) initialMap<Serial>(*pr, keys1, keys2, matches12, P3D, inv_level_sigma2, scale_factors, nlevels, *out, points, diag);
    else initialMap<Defined>(*pr, keys1, keys2, matches12, P3D, inv_level_sigma2, scale_factors, nlevels, *out, points, diag);
}

// the scalar pieces, for tests/cpp/schur_core_check.hip's twin in Python: Eigen's 3 x 3 inverse and the unpivoted LDLt
void initmapref_inverse3(const double* M, double* out) { inverse3(M, out); }
int initmapref_ldlt(int N, double* M, const double* b, double* x) { return ldltPlain(N, M, b, x) ? 1 : 0; }

}  // extern "C"
