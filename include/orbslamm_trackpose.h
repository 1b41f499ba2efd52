/* orbslamm_trackpose.h -- the block of liborbslamm_hip.so's C ABI that closes Tracking::TrackLocalMap and
 * Tracking::TrackWithMotionModel and Tracking::TrackReferenceKeyFrame (section 8t) on the device.  Included by orbslamm_hip.h, whose types it uses
 * (orbm_t, orbm_frameset_t, orbw_pool_t, orbu_store_t, OrboFrame, OrboResult, the ORBX_* codes); including either gives both. */
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

/* ---------------------------------------------------------------------------------------------------------------------
 * Tracking::TrackReferenceKeyFrame (Tracking.cc:802-844), from SearchByBoW to the loop behind PoseOptimization, for any number of
 * (keyframe, frame) pairs in ONE call; with solve = 0 the first loop of Tracking::Relocalization
 * (Tracking.cc:1428-1449: one lost frame against every candidate keyframe).  Everything read is resident: both frames'
 * descriptors, angles, FeatureVectors and mvKeysUn in the frame set, the keyframe's match list in the keyframe store, the
 * points' bad bit and positions in the pool.
 *
 * Validity (ORBmatcher.cc:191-197: if(!pMP) continue; if(pMP->isBad()) continue;): keyframe feature q takes part when
 *   e = entries[kf][q] is not -1 and the pool record of e & ~ORBU_ENTRY_NO_VOTE carries no ORBW_FLAG_BAD.  An entry with
 *   ORBU_ENTRY_NO_VOTE is a point in the match slot: it takes part.  A feature at or above the store's stride holds no point.
 *   The keyframe's own bad flag is not consulted (Relocalization tests it before the call, :1431: that stays with the caller).
 * Search (ORBmatcher.cc:159-290): orbm_bow_frames' search with that validity, TH_LOW = 50 (:214), the call's nnratio (:220; 0.7
 *   at Tracking.cc:808, 0.75 at :1425) and check_ori (:222-233, :268-287).  match[t] = the keyframe feature matched to frame
 *   feature t, or -1, behind the rotation pruning; n_bow its count over t < n (the nmatches :289 returns when n is the slot's
 *   feature count, mCurrentFrame.N; the search itself always runs over the whole slot, and with a smaller n the features behind
 *   n take no part in the count, the gate, the merge or the solve).  With every feature valid the table is the one
 *   orbm_bow_frames returns for the pair.
 * Merge (ORBmatcher.cc:236 vpMapPointMatches[bestIdxF]=pMP; Tracking.cc:817 mCurrentFrame.mvpMapPoints = vpMapPointMatches):
 *   merged[t] = entries[kf][match[t]] with bit 30 cleared where match[t] >= 0, else -1.  There are no base ids: the assignment
 *   replaces mvpMapPoints whole.
 * Gate (Tracking.cc:814 if(nmatches<15) return false; :1436 if(nmatches<15) { vbDiscarded[i] = true; continue; }): n_bow <
 *   min_matches gives status ORBQ_REF_TOO_FEW (the reference's value is 15); else solve = 0 gives ORBQ_REF_SEARCH_ONLY.  In both
 *   no solve runs: track.opt is zero but for Tcw, the pose as it came; ids_out[t] = merged[t], outlier_out[t] = 0,
 *   n_matches = n_bow, n_matches_map = 0.  (The reference returns before it touches the frame: a drop-in must not write it.)
 * Solve and loop (Tracking.cc:818-841): otherwise orbq_track_pose's path with discard = 1 -- the edges in ascending t (:818
 *   SetPose(mLastFrame.mTcw) is job.frame, :820 PoseOptimization), the loop of :824-841 (the same as :950-969): an outlier gets
 *   ids_out[t] = -1 (:832) and keeps its byte at 1; n_matches, n_matches_map from the pool's observed bit (:838-839).  Status
 *   ORBQ_REF_TRACKED.  The verdict nmatchesMap >= 10 (:843) is the caller's.
 * The call: synchronous, one synchronise; one packed upload (the job records) and one copy down (results | ids | outlier bytes |
 *   the match tables that were asked for); nothing per feature or per match goes up.  Jobs may name different frame sets of h,
 *   the same keyframe or the same frame several times; a job's bytes do not depend on its neighbours, and the same call twice
 *   gives the same bytes.  The scratch is the handle's own: no result set of the frame set's BoW ring is taken or disturbed.
 *   The pool's mutex (the store shares it) is held from the checks to the synchronise, and the call leaves the reader event
 *   orbw_pool_set* and orbu_* wait for.  It runs on the handle's stream, behind the slots' builds and
 *   orbm_frameset_compute_bow as orbm_bow_frames does.
 * match_out may be null, or hold nulls: those tables are not copied down.
 * Refusals (never truncations; the argument checks come first and need no GPU):
 *   n_jobs == 0: ORBX_OK at once.
 *   ORBX_E_UNSUPPORTED above ORBO_MAX_FRAMES jobs, n above ORBO_MAX_EDGES, more than ORBO_MAX_CALL_EDGES features a call, or jobs
 *   whose frame sets' caps add up to more than ORBO_MAX_CALL_EDGES (the search's scratch is 11 bytes a feature of the cap).
 *   ORBX_E_INVALID for null arguments, n < 0 or above the set's cap, solve outside {0, 1}, min_matches < 0, nlevels outside
 *   [1, 16], a slot outside the set, a frame set of another handle, a store of another pool, kf outside the store or not set,
 *   orbm_frameset_compute_bow has not run; and, found by the kernel and reported behind it with the outputs unwritten: an
 *   edge's octave outside [0, nlevels), or a feature with a point at or above the slot's device count.
 *   No CPU fallback. */
typedef struct {
    orbm_frameset_t* fs;
    int32_t kf_slot;   /* the reference keyframe as a slot of fs: descriptors, angles, FeatureVector */
    int32_t slot;      /* mCurrentFrame */
    int32_t kf;        /* the keyframe's slot in the store: entries[kf][q] = pool id of its feature q */
    int32_t n;         /* mCurrentFrame.N */
    int32_t solve;     /* 1: TrackReferenceKeyFrame; 0: the search and the merge only (Relocalization's first loop) */
    OrboFrame frame;   /* mLastFrame.mTcw and K, as orbo_* take them (read when solve = 1) */
} OrbqRefJob;
#define ORBQ_REF_TRACKED 0
#define ORBQ_REF_TOO_FEW 1
#define ORBQ_REF_SEARCH_ONLY 2
typedef struct { OrbqResult track; int32_t n_bow; int32_t status; } OrbqRefResult;
int orbq_track_reference(orbm_t* h, orbw_pool_t* pool, orbu_store_t* store, const OrbqRefJob* jobs, int n_jobs,
                         float nnratio, int check_ori, int min_matches,
                         const float* inv_level_sigma2, int nlevels, OrbqRefResult* out,
                         int32_t* const* ids_out, uint8_t* const* outlier_out, int32_t* const* match_out /* may be null, or hold nulls */);

#ifdef __cplusplus
}
#endif
#endif
