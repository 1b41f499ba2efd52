// init_ref_capi.cpp -- C entry points over the Initializer restatement (tools/init_ref.hpp) for the tests (ctypes);
// built with g++ -ffp-contract=off by tests/init_cases.py.
#include <cstring>
#include <vector>

#include "../../tools/init_ref.hpp"

using init_ref::KeyPt;

extern "C" {

// Initializer(keys1, K, sigma, iters) + Initialize(keys2, m12, sets): p3d / tri hold the caller's vP3D / vbTriangulated
// and are written only where the reference writes them
int initref_initialize(const KeyPt* k1, int n1, const KeyPt* k2, int n2, const float* K, float sigma, int iters, int hf,
                       const int32_t* m12, const int32_t* sets, init_ref::Result* res, float* p3d, uint8_t* tri)
{
    init_ref::Initializer ini(std::vector<KeyPt>(k1, k1 + n1), K, sigma, iters, hf != 0);
    std::vector<float> P(p3d, p3d + (size_t)n1 * 3);
    std::vector<uint8_t> T(tri, tri + n1);
    const std::vector<int> m(m12, m12 + n1);
    const std::vector<int32_t> s(sets, sets + (size_t)iters * 8);
    const bool ok = ini.Initialize(std::vector<KeyPt>(k2, k2 + n2), m, s, *res, P, T);
    std::memcpy(p3d, P.data(), P.size() * sizeof(float));
    std::memcpy(tri, T.data(), T.size());
    return ok ? 1 : 0;
}

// cv::SVD::compute(a, w, u, vt, full ? FULL_UV : 0) on a rows x cols CV_32F; dims = (len w, u rows, u cols, vt rows, vt cols)
void initref_svd(const float* a, int rows, int cols, int full, float* w, float* u, float* vt, int32_t* dims)
{
    init_ref::Mat A(rows, cols), W, U, Vt;
    std::memcpy(A.d.data(), a, sizeof(float) * rows * cols);
    init_ref::svd(A, full != 0, W, U, Vt);
    std::memcpy(w, W.d.data(), W.d.size() * sizeof(float));
    std::memcpy(u, U.d.data(), U.d.size() * sizeof(float));
    std::memcpy(vt, Vt.d.data(), Vt.d.size() * sizeof(float));
    dims[0] = W.rows; dims[1] = U.rows; dims[2] = U.cols; dims[3] = Vt.rows; dims[4] = Vt.cols;
}

// Normalize: T (3x3) and the normalised points (n x 2)
void initref_normalize(const KeyPt* k, int n, float* T9, float* pn)
{
    std::vector<float> P;
    init_ref::Mat T;
    init_ref::Initializer::Normalize(std::vector<KeyPt>(k, k + n), P, T);
    std::memcpy(T9, T.d.data(), 9 * sizeof(float));
    std::memcpy(pn, P.data(), P.size() * sizeof(float));
}

// Initialize's set drawing through DUtils::Random (SeedRandOnce(0): seeds only at the first call in the process)
void initref_draw_sets(int n, int iters, int32_t* out)
{
    const std::vector<int32_t> s = init_ref::drawSets(n, iters);
    std::memcpy(out, s.data(), s.size() * sizeof(int32_t));
}

int initref_random_int(int lo, int hi) { return init_ref::randomInt(lo, hi); }

}  // extern "C"
