// pnp_ref.hpp -- an independent restatement of PnPsolver (src/PnPsolver.cc; `ref:LINE` cites it) for the tests and for
// tools/pnp_bench.py: EPnP under RANSAC as Tracking::Relocalization uses it, on the host, in plain C++ with the standard
// library alone.  It shares no header with the library (orbx_cvmath.hpp included): the OpenCV 3.0 pieces the reference
// calls -- cvMulTransposed(order 1), cvSVD / cvInvert(CV_SVD) / cvSolve(CV_SVD) over JacobiSVDImpl_<double> and SVBkSb,
// convertTo 64F -> 32F -- are restated here on their own, unpinned as DESIGN.md §2 says of all the others.  Build with
// -ffp-contract=off: one IEEE operation per source operation.
//
// The RANSAC sets are an input (the reference draws them inside iterate; drawSets draws them the same way up front).
// Defined choices, the same as the device's: gauss_newton's X starts as zeros; qr_solve prints nothing;
// min_set != 4 and N == 0 are refused; the double -> int conversion of the iteration count is x86's; the hypot of the
// Jacobi rotations is lapack.cpp's template, in binary64; a NaN of compute_pose's R and t leaves as x86's default NaN.
#pragma once

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cv_ref.hpp"

namespace pnp_ref {

// ------------------------------------------------------------------ OpenCV 3.0, binary64
using cv_ref::hypotCv;   // lapack.cpp's hypot, in binary64 here

// JacobiSVDImpl_<double>(At, W, Vt, m, n, n1 = n, DBL_MIN, DBL_EPSILON*10): At holds n rows of m (the transposed source),
// on return row i is the i-th left singular vector; Vt (n x n) row i the i-th right one; W descending.
inline void jacobiSVD(double* At, int m, int n, double* W, double* Vt)
{
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    const int maxIter = m > 30 ? m : 30;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
        Vt[i * n + i] = 1;
    }
    for (int iter = 0; iter < maxIter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double* Ai = At + i * m;
                double* Aj = At + j * m;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (std::fabs(p) <= eps * std::sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = hypotCv(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = std::sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = std::sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const double t0 = c * Ai[k] + s * Aj[k];
                    const double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += t0 * t0; b += t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                double* Vi = Vt + i * n;
                double* Vj = Vt + j * n;
                for (int k = 0; k < n; k++) {
                    const double t0 = c * Vi[k] + s * Vj[k];
                    const double t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            for (int k = 0; k < m; k++) std::swap(At[i * m + k], At[j * m + k]);
            for (int k = 0; k < n; k++) std::swap(Vt[i * n + k], Vt[j * n + k]);
        }
    }
    // a zero singular value: its left vector is a random one, orthogonalised (cv::RNG(0x12345678))
    uint64_t state = 0x12345678;
    for (int i = 0; i < n; i++) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const double val0 = 1. / m;
            for (int k = 0; k < m; k++) {
                state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
                At[i * m + k] = ((unsigned)state & 256) != 0 ? val0 : -val0;
            }
            for (int it = 0; it < 2; it++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    double asum = 0;
                    for (int k = 0; k < m; k++) {
                        const double t = At[i * m + k] - sd * At[j * m + k];
                        At[i * m + k] = t;
                        asum += std::fabs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
            sd = std::sqrt(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

// cvSVD(A, W, U, V, flags) of an m x n matrix (m >= n, row-major): Ut (n x m) rows = left vectors, Vt (n x n)
inline void svd(const double* A, int m, int n, double* W, double* Ut, double* Vt)
{
    for (int i = 0; i < n; i++) for (int k = 0; k < m; k++) Ut[i * m + k] = A[k * n + i];
    jacobiSVD(Ut, m, n, W, Vt);
}

// SVBkSbImpl_<double> with eps = DBL_EPSILON*2: x (n x nb) = V * diag(1/w) * U^T * b; b == null: the identity (nb = m)
inline void svBkSb(int m, int n, const double* w, const double* Ut, const double* Vt, const double* b, int nb, double* x)
{
    const int nm = m < n ? m : n;
    if (!b) nb = m;
    for (int i = 0; i < n * nb; i++) x[i] = 0;
    double threshold = 0;
    for (int i = 0; i < nm; i++) threshold += w[i];
    threshold *= DBL_EPSILON * 2;
    std::vector<double> buffer(nb);
    for (int i = 0; i < nm; i++) {
        double wi = w[i];
        if (std::fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        if (nb == 1) {
            double s = 0;
            if (b) for (int j = 0; j < m; j++) s += Ut[i * m + j] * b[j];
            else s = Ut[i * m];
            s *= wi;
            for (int j = 0; j < n; j++) x[j] = x[j] + s * Vt[i * n + j];
        } else {
            if (b) {
                for (int j = 0; j < nb; j++) buffer[j] = 0;
                for (int r = 0; r < m; r++) { const double s = Ut[i * m + r]; for (int j = 0; j < nb; j++) buffer[j] = buffer[j] + s * b[r * nb + j]; }
                for (int j = 0; j < nb; j++) buffer[j] *= wi;
            } else
                for (int j = 0; j < nb; j++) buffer[j] = Ut[i * m + j] * wi;
            for (int r = 0; r < n; r++) { const double s = Vt[i * n + r]; for (int j = 0; j < nb; j++) x[r * nb + j] = x[r * nb + j] + s * buffer[j]; }
        }
    }
}

// cvInvert(A, Ainv, CV_SVD), 3x3 (a pseudo-inverse when a singular value falls under the threshold)
inline void invert3(const double* A, double* Ainv)
{
    double W[3], Ut[9], Vt[9];
    svd(A, 3, 3, W, Ut, Vt);
    svBkSb(3, 3, W, Ut, Vt, nullptr, 3, Ainv);
}

// cvSolve(A, b, x, CV_SVD), A m x n with m >= n, one right-hand side
inline void solveSVD(const double* A, int m, int n, const double* b, double* x)
{
    double W[8], Ut[64], Vt[64];
    svd(A, m, n, W, Ut, Vt);
    svBkSb(m, n, W, Ut, Vt, b, 1, x);
}

// cvMulTransposed(src, dst, 1): dst = src^T * src, src rows x cols.  MulTransposedR: each entry of the upper triangle one
// sum over the rows in order, times the scale 1; completeSymm mirrors it.
inline void mulTransposed(const double* src, int rows, int cols, double* dst)
{
    for (int i = 0; i < cols; i++)
        for (int j = i; j < cols; j++) {
            double s = 0;
            for (int k = 0; k < rows; k++) s += src[k * cols + i] * src[k * cols + j];
            dst[i * cols + j] = s * 1.0;
        }
    for (int i = 0; i < cols; i++) for (int j = 0; j < i; j++) dst[i * cols + j] = dst[j * cols + i];
}

// ------------------------------------------------------------------ EPnP (ref:342-950)
inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline double dist2(const double* a, const double* b)
{
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// qr_solve (ref:860-950) on a 6 x 4 system, in place; false: the singular branch (X untouched, nothing printed)
inline bool qrSolve(double* A, double* b, double* X)
{
    const int nr = 6, nc = 4;
    double A1[6], A2[6];
    for (int k = 0; k < nc; k++) {
        double* akk = A + k * nc + k;
        // the scan reads rows k .. nr-2 (its pointer starts at row k while its counter starts at k+1): kept
        double eta = std::fabs(*akk);
        for (int i = k + 1; i < nr; i++) { const double elt = std::fabs(akk[(i - k - 1) * nc]); if (eta < elt) eta = elt; }
        if (eta == 0) { A1[k] = A2[k] = 0.0; return false; }
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) { akk[(i - k) * nc] *= inv_eta; sum += akk[(i - k) * nc] * akk[(i - k) * nc]; }
        double sigma = std::sqrt(sum);
        if (*akk < 0) sigma = -sigma;
        *akk += sigma;
        A1[k] = sigma * *akk;
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s = 0;
            for (int i = k; i < nr; i++) s += akk[(i - k) * nc] * akk[(i - k) * nc + (j - k)];
            const double tau = s / A1[k];
            for (int i = k; i < nr; i++) akk[(i - k) * nc + (j - k)] -= tau * akk[(i - k) * nc];
        }
    }
    for (int j = 0; j < nc; j++) {
        const double* ajj = A + j * nc + j;
        double tau = 0;
        for (int i = j; i < nr; i++) tau += ajj[(i - j) * nc] * b[i];
        tau /= A1[j];
        for (int i = j; i < nr; i++) b[i] -= tau * ajj[(i - j) * nc];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double s = 0;
        for (int j = i + 1; j < nc; j++) s += A[i * nc + j] * X[j];
        X[i] = (b[i] - s) / A2[i];
    }
    return true;
}

inline double nanCanonical(double v)
{
    if (v == v) return v;
    const uint64_t bits = 0xFFF8000000000000ull;
    std::memcpy(&v, &bits, sizeof v);
    return v;
}

struct Camera { double fu, fv, uc, vc; };   // double members holding the frame's floats (ref:104-107)

class Epnp {
public:
    Camera cam;
    std::vector<double> pws, us, alphas, pcs;
    int n = 0;
    double cws[4][3], ccs[4][3];

    void reset() { n = 0; pws.clear(); us.clear(); }
    void add(double X, double Y, double Z, double u, double v)
    {
        pws.push_back(X); pws.push_back(Y); pws.push_back(Z);
        us.push_back(u); us.push_back(v);
        n++;
    }

    void chooseControlPoints()   // ref:375-409
    {
        cws[0][0] = cws[0][1] = cws[0][2] = 0;
        for (int i = 0; i < n; i++) for (int j = 0; j < 3; j++) cws[0][j] += pws[3 * i + j];
        for (int j = 0; j < 3; j++) cws[0][j] /= n;
        std::vector<double> pw0((size_t)3 * n);
        for (int i = 0; i < n; i++) for (int j = 0; j < 3; j++) pw0[3 * i + j] = pws[3 * i + j] - cws[0][j];
        double ptp[9], dc[3], uct[9], vt[9];
        mulTransposed(pw0.data(), n, 3, ptp);
        svd(ptp, 3, 3, dc, uct, vt);
        for (int i = 1; i < 4; i++) {
            const double k = std::sqrt(dc[i - 1] / n);
            for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * uct[3 * (i - 1) + j];
        }
    }

    void barycentric()   // ref:411-434
    {
        double cc[9], ci[9];
        for (int i = 0; i < 3; i++) for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
        invert3(cc, ci);
        alphas.resize((size_t)4 * n);
        for (int i = 0; i < n; i++) {
            const double* pi = &pws[3 * i];
            double* a = &alphas[4 * i];
            for (int j = 0; j < 3; j++)
                a[1 + j] = ci[3 * j] * (pi[0] - cws[0][0]) + ci[3 * j + 1] * (pi[1] - cws[0][1]) + ci[3 * j + 2] * (pi[2] - cws[0][2]);
            a[0] = 1.0f - a[1] - a[2] - a[3];
        }
    }

    void computeL(const double* ut, double* L) const   // ref:760-800
    {
        const double* v[4] = {ut + 12 * 11, ut + 12 * 10, ut + 12 * 9, ut + 12 * 8};
        double dv[4][6][3];
        for (int i = 0; i < 4; i++) {
            int a = 0, b = 1;
            for (int j = 0; j < 6; j++) {
                for (int c = 0; c < 3; c++) dv[i][j][c] = v[i][3 * a + c] - v[i][3 * b + c];
                b++;
                if (b > 3) { a++; b = a + 1; }
            }
        }
        for (int i = 0; i < 6; i++) {
            double* row = L + 10 * i;
            row[0] = dot3(dv[0][i], dv[0][i]);
            row[1] = 2.0f * dot3(dv[0][i], dv[1][i]);
            row[2] = dot3(dv[1][i], dv[1][i]);
            row[3] = 2.0f * dot3(dv[0][i], dv[2][i]);
            row[4] = 2.0f * dot3(dv[1][i], dv[2][i]);
            row[5] = dot3(dv[2][i], dv[2][i]);
            row[6] = 2.0f * dot3(dv[0][i], dv[3][i]);
            row[7] = 2.0f * dot3(dv[1][i], dv[3][i]);
            row[8] = 2.0f * dot3(dv[2][i], dv[3][i]);
            row[9] = dot3(dv[3][i], dv[3][i]);
        }
    }

    // find_betas_approx_1 / 2 / 3 (ref:667-758): the columns of L they keep, then the closed forms
    static void betasApprox(int which, const double* L, const double* rho, double* betas)
    {
        static const int cols1[4] = {0, 1, 3, 6}, cols23[5] = {0, 1, 2, 3, 4};
        const int nc = which == 1 ? 4 : which == 2 ? 3 : 5;
        const int* cols = which == 1 ? cols1 : cols23;
        double l[30], b[5];
        for (int i = 0; i < 6; i++) for (int c = 0; c < nc; c++) l[i * nc + c] = L[10 * i + cols[c]];
        solveSVD(l, 6, nc, rho, b);
        if (which == 1) {
            if (b[0] < 0) {
                betas[0] = std::sqrt(-b[0]);
                betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0];
            } else {
                betas[0] = std::sqrt(b[0]);
                betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0];
            }
            return;
        }
        if (b[0] < 0) {
            betas[0] = std::sqrt(-b[0]);
            betas[1] = (b[2] < 0) ? std::sqrt(-b[2]) : 0.0;
        } else {
            betas[0] = std::sqrt(b[0]);
            betas[1] = (b[2] > 0) ? std::sqrt(b[2]) : 0.0;
        }
        if (b[1] < 0) betas[0] = -betas[0];
        betas[2] = which == 3 ? b[3] / betas[0] : 0.0;
        betas[3] = 0.0;
    }

    static void gaussNewton(const double* L, const double* rho, double* betas)   // ref:812-858
    {
        double A[24], b[6], x[4] = {0, 0, 0, 0};   // (defined: the reference leaves x uninitialised)
        for (int k = 0; k < 5; k++) {
            for (int i = 0; i < 6; i++) {
                const double* r = L + i * 10;
                double* a = A + i * 4;
                a[0] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3];
                a[1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3];
                a[2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3];
                a[3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3];
                b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] +
                                 r[3] * betas[0] * betas[2] + r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] +
                                 r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] + r[8] * betas[2] * betas[3] +
                                 r[9] * betas[3] * betas[3]);
            }
            qrSolve(A, b, x);
            for (int i = 0; i < 4; i++) betas[i] += x[i];
        }
    }

    double reprojectionError(const double R[9], const double t[3]) const   // ref:550-567
    {
        double sum2 = 0.0;
        for (int i = 0; i < n; i++) {
            const double* pw = &pws[3 * i];
            const double Xc = dot3(R, pw) + t[0];
            const double Yc = dot3(R + 3, pw) + t[1];
            const double inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
            const double ue = cam.uc + cam.fu * Xc * inv_Zc;
            const double ve = cam.vc + cam.fv * Yc * inv_Zc;
            const double u = us[2 * i], v = us[2 * i + 1];
            sum2 += std::sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
        }
        return sum2 / n;
    }

    void estimateRt(double R[9], double t[3]) const   // ref:569-627
    {
        double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
        for (int i = 0; i < n; i++)
            for (int j = 0; j < 3; j++) { pc0[j] += pcs[3 * i + j]; pw0[j] += pws[3 * i + j]; }
        for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
        double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, d[3], ut[9], vt[9];
        for (int i = 0; i < n; i++) {
            const double* pc = &pcs[3 * i];
            const double* pw = &pws[3 * i];
            for (int j = 0; j < 3; j++) {
                abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
                abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
                abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
            }
        }
        svd(abt, 3, 3, d, ut, vt);
        // U and V untransposed: U(i, k) = ut[k][i], V(j, k) = vt[k][j]; R(i, j) = row i of U . row j of V
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[3 * i + j] = ut[i] * vt[j] + ut[3 + i] * vt[3 + j] + ut[6 + i] * vt[6 + j];
        const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
        if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
        t[0] = pc0[0] - dot3(R, pw0);
        t[1] = pc0[1] - dot3(R + 3, pw0);
        t[2] = pc0[2] - dot3(R + 6, pw0);
    }

    double computeRt(const double* ut, const double* betas, double R[9], double t[3])   // ref:651-662
    {
        for (int i = 0; i < 4; i++) ccs[i][0] = ccs[i][1] = ccs[i][2] = 0.0f;
        for (int i = 0; i < 4; i++) {
            const double* v = ut + 12 * (11 - i);
            for (int j = 0; j < 4; j++) for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[3 * j + k];
        }
        pcs.resize((size_t)3 * n);
        for (int i = 0; i < n; i++) {
            const double* a = &alphas[4 * i];
            for (int j = 0; j < 3; j++) pcs[3 * i + j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
        }
        if (pcs[2] < 0.0) {   // solve_for_sign: the first point's depth only
            for (int i = 0; i < 4; i++) for (int j = 0; j < 3; j++) ccs[i][j] = -ccs[i][j];
            for (size_t i = 0; i < pcs.size(); i++) pcs[i] = -pcs[i];
        }
        estimateRt(R, t);
        return reprojectionError(R, t);
    }

    double computePose(double R[9], double t[3])   // ref:477-525
    {
        chooseControlPoints();
        barycentric();
        std::vector<double> M((size_t)2 * n * 12);
        for (int i = 0; i < n; i++) {
            const double* as = &alphas[4 * i];
            const double u = us[2 * i], v = us[2 * i + 1];
            double* M1 = &M[(size_t)2 * i * 12];
            double* M2 = M1 + 12;
            for (int k = 0; k < 4; k++) {
                M1[3 * k] = as[k] * cam.fu; M1[3 * k + 1] = 0.0; M1[3 * k + 2] = as[k] * (cam.uc - u);
                M2[3 * k] = 0.0; M2[3 * k + 1] = as[k] * cam.fv; M2[3 * k + 2] = as[k] * (cam.vc - v);
            }
        }
        double mtm[144], d[12], ut[144], vt[144];
        mulTransposed(M.data(), 2 * n, 12, mtm);
        svd(mtm, 12, 12, d, ut, vt);
        double L[60], rho[6];
        computeL(ut, L);
        rho[0] = dist2(cws[0], cws[1]); rho[1] = dist2(cws[0], cws[2]); rho[2] = dist2(cws[0], cws[3]);
        rho[3] = dist2(cws[1], cws[2]); rho[4] = dist2(cws[1], cws[3]); rho[5] = dist2(cws[2], cws[3]);
        double betas[4][4], err[4], Rs[4][9], ts[4][3];
        for (int w = 1; w <= 3; w++) {
            betasApprox(w, L, rho, betas[w]);
            gaussNewton(L, rho, betas[w]);
            err[w] = computeRt(ut, betas[w], Rs[w], ts[w]);
        }
        int N = 1;
        if (err[2] < err[1]) N = 2;
        if (err[3] < err[N]) N = 3;
        // a NaN leaves as one pattern (x86's default NaN): which of two NaN operands an operation hands on is the
        // compiler's choice of operand order, not the source's (defined)
        for (int k = 0; k < 9; k++) R[k] = nanCanonical(Rs[N][k]);
        for (int k = 0; k < 3; k++) t[k] = nanCanonical(ts[N][k]);
        return err[N];
    }
};

// ------------------------------------------------------------------ RANSAC (ref:67-339)
struct Hypothesis {
    int32_t n_inliers;        // mnInliersi
    int32_t is_record;        // it became the running best (count >= min and > mnBestInliers)
    int32_t refine_inliers;   // is_record: mnRefinedInliers of Refine() on its mask
    int32_t refine_ok;        // is_record: Refine()'s return
    double R[9], t[3];        // mRi, mti
    double refine_R[9], refine_t[3];
};

struct Result {
    int32_t returned, no_more, n_inliers, hypothesis, refined, iterations, best_inliers, best_hypothesis;
    float Tcw[16], best_Tcw[16];
};

// the draw of ref:191-201: `iters` sets of 4
inline std::vector<int32_t> drawSets(int n, int iters) { return cv_ref::drawSets(n, iters, 4); }

class PnPsolver {
public:
    static const int kCapacity = -4, kUnsupported = -5;

    PnPsolver(int nAll, const int32_t* idx, int n, const float* P2D, const float* sigma2, const float* P3Dw, const float K[4])
        : nAll_(nAll), N(n), idx_(idx, idx + n), p2d_(P2D, P2D + 2 * (size_t)n), sigma2_(sigma2, sigma2 + n), p3d_(P3Dw, P3Dw + 3 * (size_t)n)
    {
        epnp_.cam.fu = K[0]; epnp_.cam.fv = K[1]; epnp_.cam.uc = K[2]; epnp_.cam.vc = K[3];
        SetRansacParameters(0.99, 8, 300, 4, 0.4f, 5.991f);
    }

    int SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2)   // ref:121-157
    {
        if (minSet != 4 || N == 0) return kUnsupported;
        prob_ = probability; minInliers_ = minInliers; maxIts_ = maxIterations; eps_ = epsilon;
        inl_.assign(N, 0);
        int nMin = (int)(N * eps_);
        if (nMin < minInliers_) nMin = minInliers_;
        if (nMin < minSet) nMin = minSet;
        minInliers_ = nMin;
        if (eps_ < (float)minInliers_ / N) eps_ = (float)minInliers_ / N;
        int nIterations;
        if (minInliers_ == N)
            nIterations = 1;
        else {
            const double v = std::ceil(std::log(1 - prob_) / std::log(1 - std::pow((double)eps_, 3.0)));
            nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
        }
        maxIts_ = std::max(1, std::min(nIterations, maxIts_));
        maxErr_.resize(N);
        for (int i = 0; i < N; i++) maxErr_[i] = sigma2_[i] * th2;
        return 0;
    }

    int maxIterations() const { return maxIts_; }
    int minInliers() const { return minInliers_; }
    float epsilon() const { return eps_; }
    int iterations() const { return its_; }
    int size() const { return N; }
    float maxError(int i) const { return maxErr_[i]; }

    void checkInliers()   // ref:308-339
    {
        nInl_ = 0;
        const double fu = epnp_.cam.fu, fv = epnp_.cam.fv, uc = epnp_.cam.uc, vc = epnp_.cam.vc;
        for (int i = 0; i < N; i++) {
            const float X = p3d_[3 * i], Y = p3d_[3 * i + 1], Z = p3d_[3 * i + 2];
            const float Xc = Ri_[0] * X + Ri_[1] * Y + Ri_[2] * Z + ti_[0];
            const float Yc = Ri_[3] * X + Ri_[4] * Y + Ri_[5] * Z + ti_[1];
            const float invZc = 1 / (Ri_[6] * X + Ri_[7] * Y + Ri_[8] * Z + ti_[2]);
            const double ue = uc + fu * Xc * invZc;
            const double ve = vc + fv * Yc * invZc;
            const float distX = p2d_[2 * i] - ue;
            const float distY = p2d_[2 * i + 1] - ve;
            const float error2 = distX * distX + distY * distY;
            if (error2 < maxErr_[i]) { inl_[i] = 1; nInl_++; }
            else inl_[i] = 0;
        }
    }

    bool Refine()   // ref:260-305
    {
        epnp_.reset();
        for (int i = 0; i < N; i++)
            if (bestInl_[i]) epnp_.add(p3d_[3 * i], p3d_[3 * i + 1], p3d_[3 * i + 2], p2d_[2 * i], p2d_[2 * i + 1]);
        epnp_.computePose(Ri_, ti_);
        checkInliers();
        nRefined_ = nInl_;
        refinedInl_ = inl_;
        if (nInl_ > minInliers_) { toTcw(refinedTcw_); return true; }
        return false;
    }

    // iterate (ref:165-258) over the sets given: set k (4 indices) is the draw of iteration k.  hyp (may be null): entry k
    // receives hypothesis k as it is evaluated.  stopOnRefine false: a successful Refine does not return (every hypothesis
    // of the call is evaluated; the result is then the exhaustion branch's).  kCapacity: the loop would pass nSets, the
    // solver's state is as before the call.
    int iterate(int nIterations, const int32_t* sets, int nSets, Result& res, uint8_t* inliers, Hypothesis* hyp, bool stopOnRefine = true)
    {
        std::memset(&res, 0, sizeof res);
        res.hypothesis = -1;
        if (nAll_) std::memset(inliers, 0, nAll_);
        if (N < minInliers_) { res.no_more = 1; fill(res); return 0; }
        const PnPsolver saved = *this;
        int cur = 0;
        while (its_ < maxIts_ || cur < nIterations) {
            if (its_ >= nSets) { *this = saved; res.best_hypothesis = -1; return kCapacity; }
            cur++;
            its_++;
            const int32_t* set = sets + (size_t)(its_ - 1) * 4;
            epnp_.reset();
            for (int j = 0; j < 4; j++) {
                const int i = set[j];
                epnp_.add(p3d_[3 * i], p3d_[3 * i + 1], p3d_[3 * i + 2], p2d_[2 * i], p2d_[2 * i + 1]);
            }
            epnp_.computePose(Ri_, ti_);
            checkInliers();
            Hypothesis* h = hyp ? hyp + (its_ - 1) : nullptr;
            if (h) {
                std::memset(h, 0, sizeof *h);
                h->n_inliers = nInl_;
                std::memcpy(h->R, Ri_, sizeof Ri_); std::memcpy(h->t, ti_, sizeof ti_);
            }
            if (nInl_ >= minInliers_) {
                const bool record = nInl_ > best_;
                if (record) { bestInl_ = inl_; best_ = nInl_; bestHyp_ = its_ - 1; toTcw(bestTcw_); }
                // (Refine is a pure function of the best mask: when nothing can return, only a new best needs it)
                const bool ok = (stopOnRefine || record) ? Refine() : false;
                if (h && record) {
                    h->is_record = 1; h->refine_inliers = nRefined_; h->refine_ok = ok ? 1 : 0;
                    std::memcpy(h->refine_R, Ri_, sizeof Ri_); std::memcpy(h->refine_t, ti_, sizeof ti_);
                }
                if (ok && stopOnRefine) {
                    res.returned = 1; res.refined = 1; res.n_inliers = nRefined_; res.hypothesis = its_ - 1;
                    for (int i = 0; i < N; i++) if (refinedInl_[i]) inliers[idx_[i]] = 1;
                    std::memcpy(res.Tcw, refinedTcw_, sizeof refinedTcw_);
                    fill(res);
                    return 0;
                }
            }
        }
        if (its_ >= maxIts_) {
            res.no_more = 1;
            if (best_ >= minInliers_) {
                res.returned = 1; res.n_inliers = best_; res.hypothesis = bestHyp_;
                for (int i = 0; i < N; i++) if (bestInl_[i]) inliers[idx_[i]] = 1;
                std::memcpy(res.Tcw, bestTcw_, sizeof bestTcw_);
            }
        }
        fill(res);
        return 0;
    }

    // compute_pose alone on the n correspondences given (indices into the solver's), for the unit tests
    double computePose(const int32_t* set, int n, double R[9], double t[3])
    {
        epnp_.reset();
        for (int j = 0; j < n; j++) {
            const int i = set[j];
            epnp_.add(p3d_[3 * i], p3d_[3 * i + 1], p3d_[3 * i + 2], p2d_[2 * i], p2d_[2 * i + 1]);
        }
        return epnp_.computePose(R, t);
    }

private:
    void toTcw(float T[16]) const   // convertTo(CV_32F) into eye(4, 4)
    {
        for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.f : 0.f;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)Ri_[r * 3 + c];
            T[r * 4 + 3] = (float)ti_[r];
        }
    }
    void fill(Result& r) const
    {
        r.iterations = its_; r.best_inliers = best_; r.best_hypothesis = bestHyp_;
        std::memcpy(r.best_Tcw, bestTcw_, sizeof bestTcw_);
    }

    int nAll_, N;
    std::vector<int32_t> idx_;
    std::vector<float> p2d_, sigma2_, p3d_, maxErr_;
    Epnp epnp_;
    double prob_ = 0.99, Ri_[9] = {0}, ti_[3] = {0};
    int minInliers_ = 8, maxIts_ = 300;
    float eps_ = 0.4f;
    int its_ = 0, best_ = 0, bestHyp_ = -1, nInl_ = 0, nRefined_ = 0;
    std::vector<uint8_t> inl_, bestInl_, refinedInl_;
    float bestTcw_[16] = {0}, refinedTcw_[16] = {0};
};

}  // namespace pnp_ref
