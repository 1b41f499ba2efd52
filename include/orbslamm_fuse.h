/* orbslamm_fuse.h -- the SearchInNeighbors block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (OrbmGrid, OrbxKeyPoint, orbm_t, orbm_frame_t, the ORBX_* codes); including either header
 * gives both. */
#ifndef ORBSLAMM_FUSE_H
#define ORBSLAMM_FUSE_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * LocalMapping::SearchInNeighbors (src/LocalMapping.cc:454-534), monocular: the searches of ORBmatcher::Fuse(pKF,
 * vpMapPoints, th) (ORBmatcher.cc:827-975) for MANY target keyframes in one call.  The search of one map
 * point in one target (:854-951) depends on no other pair: Fuse has no uniqueness resolve and no orientation histogram.
 * What is serial in it (isBad, IsInKeyFrame at :851, Observations, Replace, AddObservation at :953-973) is the caller's,
 * at replay; the library applies neither `bestDist <= TH_LOW` nor any edit.  Pure functions of their arguments.
 *
 * OrblFuseTarget: GetRotation, GetTranslation, GetCameraCenter (taken from the caller), K = (fx, fy, cx, cy), the image
 *   bounds of IsInImage (x >= min_x && x < max_x && y >= min_y && y < max_y) and the keyframe's grid (read by the
 *   host-array entry; the frames entry uses the resident frame's own).
 * OrblFusePoint: GetWorldPos, GetNormal, the RAW mfMinDistance / mfMaxDistance and GetDescriptor.  The library forms 0.8f *
 *   min and 1.2f * max (GetMin/MaxDistanceInvariance) and PredictScale's ratio mfMaxDistance / dist3D from the raw value.
 * Jobs: CSR over the targets: target k searches the points job_point[job_start[k] .. job_start[k + 1]) (indices into the
 *   pool; job_start[0] == 0).  A keyframe the caller lists twice is two targets or one target with two stretches of
 *   jobs: repeats are legal (the reference pushes a second neighbour once per first neighbour that lists it, :465-478).
 * OrblFuseResult, one per job entry in job order: best_idx / best_dist (-1 / 256 if none), the projection u, v, the
 *   predicted level and one ORBL_FUSE_ST_* code naming the gate that ended the pair.  u, v are 0 when the pair ended at
 *   DEPTH; level is -1 when the pair ended before PredictScale, and for LEVEL_RANGE -1 (below level 0) or nlevels (above
 *   the last; the reference reads mvScaleFactors out of bounds there).
 * Arithmetic: :855-892 in OpenCV's forms (gemm's small-matrix branch for Rcw*p3Dw+tcw, the double cv::norm, the double
 *   dot against 0.5*dist3D in double), the window, its order, the strict `<` (the first candidate in GetFeaturesInArea's
 *   order wins a tie), the level window [pred-1, pred] and (float)(e2*invSigma2) > 5.99 as orbm_window_best (chi2) has them.
 * The predicted level: PredictScale is ceil(log(ratio)/logScaleFactor) in the host's libm, which no device log equals bit
 *   for bit.  ratio -> level is a monotone step function, so orbl_level_breaks finds on the host, by bisection over the
 *   float bit patterns, for L = -1 .. nlevels-1 the largest positive finite float whose level is <= L (out[L + 1]); the
 *   kernel counts the breaks below ratio: level = #{j : ratio > breaks[j]} - 1.  A ratio that is NaN, <= breaks[0] or
 *   above breaks[nlevels] (+inf: dist3D == 0) ends at LEVEL_RANGE.  predict: the tree's own PredictScale as (ratio,
 *   log_scale_factor) -> level, for one whose log resolves to the double overload; NULL: (int)std::ceil(std::log(ratio) /
 *   log_scale_factor) in float.  Needs no GPU.
 * Limits and refusals (refused, never truncated): ORBX_E_UNSUPPORTED above ORBL_FUSE_MAX_TARGETS targets or
 *   ORBL_FUSE_MAX_JOBS job entries; ORBX_E_INVALID for more than 65535 features in a target, a job index outside the pool,
 *   a job_start that does not start at 0 or descends, a break table that does not ascend strictly, nlevels outside
 *   [1, 16], a bad grid, null arguments.  Zero targets or zero jobs: ORBX_OK, nothing written.  A target without features
 *   gives NO_CANDIDATE for every pair that passes the projection gates.  No CPU fallback. */
#define ORBL_FUSE_MAX_TARGETS 128
#define ORBL_FUSE_MAX_JOBS (1 << 22)
#define ORBL_FUSE_ST_DEPTH 0          /* p3Dc(2) < 0 (:858) */
#define ORBL_FUSE_ST_OUTSIDE_IMAGE 1  /* !IsInImage(u, v) (:869) */
#define ORBL_FUSE_ST_DISTANCE 2       /* dist3D outside [0.8 min, 1.2 max] (:880) */
#define ORBL_FUSE_ST_VIEW_ANGLE 3     /* PO.dot(Pn) < 0.5*dist3D (:886) */
#define ORBL_FUSE_ST_LEVEL_RANGE 4    /* the predicted level outside [0, nlevels) */
#define ORBL_FUSE_ST_NO_CANDIDATE 5   /* empty window, or nothing passing the level window and the chi-square test */
#define ORBL_FUSE_ST_FOUND 6
typedef struct {
    float Rcw[9], tcw[3], Ow[3], K[4];
    float min_x, max_x, min_y, max_y;
    OrbmGrid grid;
} OrblFuseTarget;
typedef struct {
    float pos[3], normal[3];
    float min_distance, max_distance;
    uint8_t desc[32];
} OrblFusePoint;
typedef struct {
    int32_t best_idx, best_dist;
    float u, v;
    int8_t level;
    uint8_t status;
    uint8_t pad[2];
} OrblFuseResult;
typedef int (*orbl_predict_fn)(float ratio, float log_scale_factor);
int orbl_level_breaks(float log_scale_factor, int nlevels, orbl_predict_fn predict, float* out /* nlevels + 1 */);
int orbl_fuse_batch(orbm_t* h, const OrblFuseTarget* targets, const OrbxKeyPoint* const* keys_un, const uint8_t* const* desc,
                    const int32_t* n, int n_targets, const OrblFusePoint* points, int n_points, const int32_t* job_start,
                    const int32_t* job_point, float th, const float* scale_factors, const float* inv_level_sigma2, int nlevels,
                    const float* level_breaks, OrblFuseResult* out);
int orbl_fuse_batch_frames(orbm_t* h, const OrblFuseTarget* targets, orbm_frame_t* const* frames, int n_targets,
                           const OrblFusePoint* points, int n_points, const int32_t* job_start, const int32_t* job_point, float th,
                           const float* scale_factors, const float* inv_level_sigma2, int nlevels, const float* level_breaks,
                           OrblFuseResult* out);

#ifdef __cplusplus
}
#endif
#endif
