/* orbslamm_initmap.h -- the initial-map block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (orbm_t, orbm_frame_t, OrbxKeyPoint, the ORBX_* codes, the ORBR_ST_* statuses of
 * orbslamm_refresh.h); including either gives both. */
#ifndef ORBSLAMM_INITMAP_H
#define ORBSLAMM_INITMAP_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * Tracking::CreateInitialMapMonocular from its bundle adjustment on (src/Tracking.cc:728-758), monocular, for any number of
 * two-keyframe maps in ONE launch: Optimizer::BundleAdjustment (src/Optimizer.cc:68-260) over the initial keyframe, the
 * current keyframe and the points they share, ComputeSceneMedianDepth(2) of the initial keyframe, the verdict of :734, and
 * the rescaling of the current pose and of every point.  A pure function of its arguments: the same call twice gives
 * identical bytes, and a problem's result does not depend on what else is in the batch.
 *
 * problems[p]: both Tcw (3x4 row-major: the rows of mTcw above its last), fx fy cx cy, fixed_first (the reference's rule is
 *   mnId == 0, :100: true for the first map of a run, false for a map made after a loss, where Levenberg's damping carries
 *   the gauge), fixed_second (0 in the reference), iterations (nIterations, [0, ORBB_MAX_ITERATIONS]; :728 passes 20), robust (bRobust; :728 leaves it true),
 *   n1 and n2 (the features of the initial and of the current frame).  matches12[p][i] (n1 of them) is mvIniMatches: the
 *   current frame's feature matched to feature i of the initial frame, or -1; P3D[p] (3 n1 floats) is mvIniP3D, read at the
 *   matched features only.  One point is made per matched feature, in ascending feature index.  orbb_initial_map takes
 *   mvKeysUn of both frames as host arrays (x, y and octave are read), orbb_initial_map_frames reads device-resident frames
 *   (their sizes are the frames': n1 and n2 of the record must equal them).  inv_level_sigma2 and scale_factors are
 *   mvInvLevelSigma2 and mvScaleFactors (nlevels floats each), shared by all problems.
 * out[p]: Tcw / Ow the adjusted poses and the camera centres KeyFrame::SetPose forms from them (orbslamm_correct.h RULE 2),
 *   Tcw2_scaled the current pose with its translation scaled (:746), median_depth / inv_median_depth (:731-732), n_points,
 *   verdict (ORBB_*), and the Levenberg run's diagnostics: iterations (calls of solve()), trials (its inner steps, summed),
 *   stop (ORBB_STOP_*), the robust chi2 at the first linearisation and at the end, the last lambda.
 * points[p][i], one record per feature of the initial frame: matched 0 leaves the record zero.  Else pos is what
 *   SetWorldPos gets behind the adjustment (:249), pos_scaled what it gets at :756, normal / min_distance / max_distance /
 *   status are UpdateNormalAndDepth at :250 (the normal / depth half of orbslamm_refresh.h over two observations -- the
 *   initial keyframe, then the current one -- with the NEW centres, the current keyframe as the reference and the current
 *   feature's octave as the level).  They are NOT rescaled: the reference does not rescale them.
 * VERDICT.  ORBB_RESET_NONFINITE: a depth of :704 is not finite (the reference's sort is undefined then: the DEFINED
 *   replacement), median_depth and inv_median_depth are the default NaN.  Else ORBB_RESET_DEPTH: median_depth < 0.  Else
 *   ORBB_RESET_TRACKED: n_points < 90 (TrackedMapPoints(1) is the point count: every point is new and carries two
 *   observations); with no point median_depth is 0 (DEFINED: the reference indexes an empty vector).  Else ORBB_OK.  With
 *   any verdict but ORBB_OK nothing is rescaled: Tcw2_scaled and pos_scaled equal the adjusted values.
 * The arithmetic is binary64 and DEFINED (tools/initmap_ref.hpp restates it and the device is held to
 *   it bit for bit): every sum over points follows one tree fixed by the point count (64 strided partials in ascending
 *   point order from +0.0, then the xor butterfly 32 .. 1), the reduced camera system is solved by an unpivoted LDLt in the
 *   poses' natural order, sin and cos are section 8o's.  Parity against g2o / Eigen is UNPINNED, as in section 8o.
 * Limits and refusals (refused, never truncated; the argument checks come before the handle's and need no GPU):
 *   ORBX_E_UNSUPPORTED above ORBB_MAX_PROBLEMS problems a call, ORBB_MAX_FEATURES features a frame, or ORBB_MAX_CALL_FEATURES
 *   features of initial frames a call (the points' scratch is 504 bytes a feature: the call's block stays below 160 MiB).
 *   ORBX_E_INVALID for null arguments, negative counts, iterations outside [0, ORBB_MAX_ITERATIONS], nlevels outside
 *   [1, 16], a non-finite pose, camera, table entry, matched position or matched key, a matches12 entry outside the second
 *   frame, a second-frame feature matched twice (SearchForInitialization never produces one), a matched key's octave
 *   outside [0, nlevels), and both poses fixed (fixed_second exists to say it: the reference never fixes the second).
 *   (With resident frames the keys live on the device: the kernel checks octave and finiteness and the call returns
 *   ORBX_E_INVALID after it, the outputs unwritten.)
 *   Zero problems: ORBX_OK at once -- no other argument is looked at and nothing is written.  No CPU fallback. */
#define ORBB_MAX_PROBLEMS 256
#define ORBB_MAX_FEATURES 65535
#define ORBB_MAX_CALL_FEATURES (1 << 18)
#define ORBB_MAX_ITERATIONS 20
#define ORBB_OK 0
#define ORBB_RESET_DEPTH 1
#define ORBB_RESET_TRACKED 2
#define ORBB_RESET_NONFINITE 3
#define ORBB_STOP_ITERATIONS 0   /* optimize() ran its nIterations (or had no vertex to optimise) */
#define ORBB_STOP_TRIALS 1       /* ten trials of one iteration were rejected */
#define ORBB_STOP_RHO_ZERO 2     /* a trial's gain was exactly zero */
#define ORBB_STOP_FLAT 3         /* _nBad >= 3: three iterations in a row gained less than a thousandth */
typedef struct { float Tcw1[12], Tcw2[12]; float K[4]; int32_t fixed_first, fixed_second, iterations, robust, n1, n2; } OrbbProblem;
typedef struct { float Tcw1[12], Tcw2[12]; float Ow1[3], Ow2[3]; float Tcw2_scaled[12]; float median_depth, inv_median_depth;
                 int32_t n_points, verdict, iterations, trials, stop, pad; double chi2_first, chi2_last, lambda; } OrbbResult;
typedef struct { float pos[3], pos_scaled[3], normal[3]; float min_distance, max_distance; uint8_t status, matched, pad[2]; } OrbbPoint;
int orbb_initial_map(orbm_t* h, const OrbbProblem* problems, int n_problems, const OrbxKeyPoint* const* keys_un1,
                     const OrbxKeyPoint* const* keys_un2, const int32_t* const* matches12, const float* const* P3D,
                     const float* inv_level_sigma2, const float* scale_factors, int nlevels, OrbbResult* out, OrbbPoint* const* points);
int orbb_initial_map_frames(orbm_t* h, const OrbbProblem* problems, int n_problems, orbm_frame_t* const* frames1,
                            orbm_frame_t* const* frames2, const int32_t* const* matches12, const float* const* P3D,
                            const float* inv_level_sigma2, const float* scale_factors, int nlevels, OrbbResult* out, OrbbPoint* const* points);

#ifdef __cplusplus
}
#endif
#endif
