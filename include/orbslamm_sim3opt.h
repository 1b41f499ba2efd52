/* orbslamm_sim3opt.h -- the OptimizeSim3 block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (orbm_t, the ORBX_* codes); including either gives both. */
#ifndef ORBSLAMM_SIM3OPT_H
#define ORBSLAMM_SIM3OPT_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * Optimizer::OptimizeSim3 (src/Optimizer.cc:1348-1543), monocular: the 7-dof Levenberg that LoopClosing::ComputeSim3 and
 * MultiMapper::Run run on every loop / merge candidate after SearchBySim3, for any number of candidates in ONE launch.  A pure
 * function of its arguments: the same call twice gives identical bytes, and a problem's result does not depend on what else is
 * in the batch.
 *
 * problems[p]: g2oS12 (q in Eigen's coefficient order x y z w, t, s), the two keyframes' GetRotation() (row-major 3x3),
 *   GetTranslation() and fx fy cx cy, th2 and bFixScale.  Problem p's correspondences are corrs[corr_start[p] ..
 *   corr_start[p + 1]): the caller does the pointer chasing of :1401-1440 (skip null and bad points and a negative
 *   GetIndexInKeyFrame) and passes the survivors in ascending i.  idx1 is i (the position in vpMatches1; carried, not read),
 *   obs1 / oct1 mvKeysUn[i] of pKF1, obs2 / oct2 mvKeysUn[i2] of pKF2, X1w / X2w the two points' GetWorldPos().  R * Xw + t is
 *   taken inside the library in float, as orbs_create takes it.  inv_level_sigma2_1 / _2 are the two keyframes'
 *   mvInvLevelSigma2 (nlevels floats each).
 * out[p]: written = 1 and q, t, s the optimised g2oS12, n_in the return value; or written = 0 on the early return of :1514
 *   (fewer than 10 correspondences left after the first check): q, t, s as they came, n_in = 0, index 1 of iterations, trials,
 *   lambda and chi2 zero.  n_corr the correspondence count, n_bad the pairs removed by the first check.  Per optimize() call:
 *   iterations (calls of the Levenberg solve), trials (its inner steps, summed), lambda and the robust chi2 at its end.
 *   removed: one byte per correspondence: 0 kept, 1 its match was nulled by the first check, 2 by the second.
 * The arithmetic is binary64 and DEFINED (tools/sim3opt_ref.hpp restates it and the device is held to it
 *   bit for bit): section 8o's summation tree over the edge index (2c for e12, 2c + 1 for e21 of correspondence c), its sin /
 *   cos, one written-down exp, g2o's numeric Jacobian (delta 1e-9, central).
 * Limits and refusals (refused, never truncated; the argument checks come before the handle's and need no GPU):
 *   ORBX_E_UNSUPPORTED above ORBZ_MAX_PROBLEMS problems a call, ORBZ_MAX_CORR correspondences a problem or ORBZ_MAX_CALL_CORR
 *   correspondences a call.
 *   ORBX_E_INVALID for null arguments, negative counts, a corr_start that does not start at 0 or descends, an octave outside
 *   [0, nlevels), nlevels outside [1, 16], a th2 that is not finite or not positive.
 *   ORBX_E_CAPACITY when the host has no memory for the call's staging.
 *   Zero problems: ORBX_OK at once -- no other argument is looked at (they may all be NULL, the handle included) and nothing
 *   is written.  No CPU fallback. */
#define ORBZ_MAX_PROBLEMS 4096
#define ORBZ_MAX_CORR 32767
#define ORBZ_MAX_CALL_CORR (1 << 21)
typedef struct {
    double q[4], t[3], s;              /* g2oS12: x y z w, Eigen's order */
    float R1w[9], t1w[3], K1[4];       /* pKF1 */
    float R2w[9], t2w[3], K2[4];       /* pKF2 */
    float th2;
    int32_t fix_scale;
} OrbzProblem;
typedef struct {
    int32_t idx1;                      /* position in vpMatches1 */
    float obs1[2]; int32_t oct1;
    float obs2[2]; int32_t oct2;
    float X1w[3], X2w[3];
} OrbzCorr;
typedef struct {
    double q[4], t[3], s;
    int32_t written, n_corr, n_bad, n_in;
    int32_t iterations[2], trials[2];
    double lambda[2], chi2[2];
} OrbzResult;
int orbz_optimize_sim3(orbm_t* h, const OrbzProblem* problems, int n_problems, const int32_t* corr_start /* n_problems + 1 */,
                       const OrbzCorr* corrs, const float* inv_level_sigma2_1, const float* inv_level_sigma2_2, int nlevels,
                       OrbzResult* out, uint8_t* removed /* one per correspondence */);

#ifdef __cplusplus
}
#endif
#endif
