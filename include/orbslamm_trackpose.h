/* orbslamm_trackpose.h -- the block of liborbslamm_hip.so's C ABI that closes Tracking::TrackLocalMap and
 * Tracking::TrackWithMotionModel on the device.  Included by orbslamm_hip.h, whose types it uses
 * (orbm_t, orbm_frameset_t, orbw_pool_t, OrboFrame, OrboResult, the ORBX_* codes); including either gives both. */
#ifndef ORBSLAMM_TRACKPOSE_H
#define ORBSLAMM_TRACKPOSE_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * Optimizer::PoseOptimization(&mCurrentFrame) as Tracking calls it right behind a pool search (Tracking.cc:947 behind
 * SearchByProjection(mCurrentFrame, mLastFrame), :990 behind SearchLocalPoints), with the loop that follows it (:950-969 or
 * :993-1013, monocular), for any number of frames in ONE launch, one wave a frame.  Nothing per matched point crosses the
 * link: the world positions are the pool's, the observations the resident frame's mvKeysUn, and the table that says which goes
 * with which is read where the search left it.
 *
 * A job: the resident current frame (fs, slot); `back`, which of the set's last searches to merge, counted as
 *   orbm_track_results counts it, or -1 for none; base_ids[t], the pool id of mvpMapPoints[t] BEFORE that search (-1 = NULL;
 *   a null array = all -1); n = mCurrentFrame.N; discard; frame = mTcw and K as orbo_* takes them.
 * PRECONDITION for back >= 0: the caller has received that search through orbm_track_results with ORBX_OK (that is where an
 *   arena overflow is replayed); a search not yet received is refused with ORBX_E_INVALID.
 * Merge (ORBmatcher.cc:121, :1440: a match overwrites): merged[t] = ids[assign[t]] where assign[t] >= 0, else base_ids[t].  The
 *   ids are the search's own: the id list of orbw_track_local_map / the last_ids of orbw_track_frame_pose as they lie in the
 *   search's staging, or the keyframe store's resident list for orbw_track_local_map_resident.
 * Edges (Optimizer.cc:302-341): one per feature t with merged[t] >= 0 in ASCENDING t; Xw is the pool record's pos, the
 *   observation mvKeysUn[t].  The pool's bad flag is not consulted (the reference does not consult it here).  The solve is
 *   orbo_pose_optimize_frames' own (section 8o): given the same edge list it returns the same bytes.
 * Out, per job: opt as OrboResult (below 3 edges: rounds 0, the pose as it came, no outlier flag).  outlier_out[j][t] =
 *   mvbOutlier[t] as PoseOptimization leaves it (0 where there is no edge).  discard = 1 (TrackWithMotionModel): an outlier
 *   feature gets ids_out[j][t] = -1 (:960) -- its byte keeps the 1, though the reference clears the flag at :961, so that
 *   the caller can set mbTrackInView / mnLastFrameSeen on that point; discard = 0 (TrackLocalMap, monocular): ids_out[j][t]
 *   = merged[t], outliers included.  n_matches = the features with a point and no outlier flag; n_matches_map = those among
 *   them whose pool record carries ORBW_FLAG_OBSERVED (nmatchesMap of :966, mnMatchesInliers of :1003; under mbOnlyTracking
 *   mnMatchesInliers is n_matches).
 * Synchronous.  Jobs may name different frame sets of the handle h.  The same call twice gives identical bytes, and a job's
 *   result does not depend on what else is in the call.  orbw_pool_set / orbw_pool_set_flags wait for the call's gather as
 *   they wait for the searches' projections.
 * Refusals (never truncations; the argument checks come before the handles' and need no GPU):
 *   n_jobs == 0: ORBX_OK at once, nothing read or written.
 *   ORBX_E_UNSUPPORTED above ORBO_MAX_FRAMES jobs, n above ORBO_MAX_EDGES, or more than ORBO_MAX_CALL_EDGES features a call.
 *   ORBX_E_INVALID for null arguments, n < 0 or above the set's cap, back outside [-1, 3], discard outside {0, 1}, nlevels
 *   outside [1, 16], a search that was not issued from a pool, not on that slot, not from this pool or not yet received, a
 *   base id outside the pool or never set; and, found by the kernel and reported behind it with the outputs unwritten: an
 *   edge's octave outside [0, nlevels), or a feature with a point at or above the slot's device count.
 *   ORBX_E_CAPACITY when the search's ids cannot be read any more: its staging was reallocated by a larger search, its slot
 *   was rebuilt, or (a resident search) the store completed another update since.
 *   No CPU fallback. */
typedef struct {
    orbm_frameset_t* fs; int32_t slot;
    int32_t back;
    const int32_t* base_ids;
    int32_t n;
    int32_t discard;
    OrboFrame frame;
} OrbqJob;
typedef struct { OrboResult opt; int32_t n_matches, n_matches_map; } OrbqResult;
int orbq_track_pose(orbm_t* h, orbw_pool_t* pool, const OrbqJob* jobs, int n_jobs, const float* inv_level_sigma2, int nlevels,
                    OrbqResult* out, int32_t* const* ids_out /* [n_jobs][n] */, uint8_t* const* outlier_out /* [n_jobs][n] */);

#ifdef __cplusplus
}
#endif
#endif
