/* orbslamm_poseopt.h -- the PoseOptimization block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (orbm_t, orbm_frame_t, OrbxKeyPoint, the ORBX_* codes); including either gives both. */
#ifndef ORBSLAMM_POSEOPT_H
#define ORBSLAMM_POSEOPT_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * Optimizer::PoseOptimization (src/Optimizer.cc:261-473), monocular: the motion-only Levenberg that Tracking runs after every
 * search (TrackWithMotionModel, TrackReferenceKeyFrame, TrackLocalMap) and Relocalization runs up to three times per
 * candidate, for any number of frames in ONE launch.  A pure function of its arguments: the same call twice gives identical
 * bytes, and a frame's result does not depend on what else is in the batch.
 *
 * frames[f]: mTcw (row-major 4x4) and fx fy cx cy.  Frame f's edges are edges[edge_start[f] .. edge_start[f + 1]), in the
 *   order of vpEdgesMono (ascending feature index in the reference; any order is taken as given): `feature` indexes the
 *   frame's mvKeysUn (x, y and octave are read), Xw is mvpMapPoints[feature]->GetWorldPos().  inv_level_sigma2 is
 *   mvInvLevelSigma2 (nlevels floats).  orbo_pose_optimize takes mvKeysUn as host arrays (keys_un[f], n_keys[f]; only the
 *   edges' observations go up), orbo_pose_optimize_frames reads device-resident frames (nothing but the edges and the poses
 *   goes up).
 * out[f]: Tcw is what SetPose would get, n_good the function's return value (nInitialCorrespondences - nBad), n_initial the
 *   edge count, rounds the rounds run (4; 1 below 10 edges; 0 below 3 edges, with n_good = 0 and the input pose returned as
 *   it came).  Per round: iterations (calls of the Levenberg solve), trials (its inner steps, summed), lambda and the robust
 *   chi2 at the round's end.  outlier: one byte per edge, mvbOutlier at the edge's feature.
 * The arithmetic is binary64 and DEFINED (tools/poseopt_ref.hpp restates it and the device is held to
 *   it bit for bit): the sums over edges follow one tree fixed by the frame's edge count (64 strided partials in ascending
 *   edge order from +0.0, then the xor butterfly 32 .. 1), x^3 is x * x * x, sin and cos are one written-down routine.
 * Limits and refusals (refused, never truncated; the argument checks come before the handle's and need no GPU):
 *   ORBX_E_UNSUPPORTED above ORBO_MAX_FRAMES frames a call, ORBO_MAX_EDGES edges a frame (a frame has at most that many
 *   features in every other entry of this library) or ORBO_MAX_CALL_EDGES edges a call (64 full frames; the call's blocks on
 *   the host and the device stay below 256 MiB).
 *   ORBX_E_INVALID for null arguments, negative counts, an edge_start that does not start at 0 or descends, a feature index
 *   outside the frame, an octave outside [0, nlevels), nlevels outside [1, 16].  (With resident frames the octaves live on
 *   the device: the kernel checks them and the call returns ORBX_E_INVALID after it, the outputs unwritten.)
 *   ORBX_E_CAPACITY when the host has no memory for the call's staging.
 *   Zero frames: ORBX_OK at once -- no other argument is looked at (they may all be NULL, the handle included) and nothing
 *   is written.  No CPU fallback. */
#define ORBO_MAX_FRAMES 4096
#define ORBO_MAX_EDGES 65535
#define ORBO_MAX_CALL_EDGES (1 << 22)
typedef struct { float Tcw[16]; float K[4]; } OrboFrame;          /* fx fy cx cy */
typedef struct { int32_t feature; float Xw[3]; } OrboEdge;        /* mvpMapPoints[feature], GetWorldPos() */
typedef struct { float Tcw[16]; int32_t n_initial, n_good, rounds; int32_t iterations[4], trials[4];
                 double lambda[4], chi2[4]; } OrboResult;
int orbo_pose_optimize(orbm_t* h, const OrboFrame* frames, const OrbxKeyPoint* const* keys_un, const int32_t* n_keys, int n_frames,
                       const int32_t* edge_start /* n_frames + 1 */, const OrboEdge* edges, const float* inv_level_sigma2, int nlevels,
                       OrboResult* out, uint8_t* outlier /* one per edge */);
int orbo_pose_optimize_frames(orbm_t* h, const OrboFrame* frames, orbm_frame_t* const* resident, int n_frames,
                              const int32_t* edge_start /* n_frames + 1 */, const OrboEdge* edges, const float* inv_level_sigma2, int nlevels,
                              OrboResult* out, uint8_t* outlier /* one per edge */);

#ifdef __cplusplus
}
#endif
#endif
