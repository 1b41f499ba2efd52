/* orbslamm_motion.h -- the block of liborbslamm_hip.so's C ABI that closes Tracking::TrackWithMotionModel on the device, from the
 * predicted pose to the counts its verdicts read.  Included by orbslamm_hip.h, whose types it uses (orbm_t,
 * orbm_frameset_t, orbw_pool_t, OrbqResult, the ORBX_* codes); including either gives both. */
#ifndef ORBSLAMM_MOTION_H
#define ORBSLAMM_MOTION_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * Tracking::TrackWithMotionModel (Tracking.cc:917-978, monocular) from :925 to :969, for any number of independent jobs in ONE
 * call.  A job is (current frame, last frame, the last frame's points, the velocity).  Everything read is resident: positions and
 * the observed bit in the map-point pool, both frames' mvKeysUn, the current frame's grid and descriptors and the last frame's
 * descriptors and angles in frame-set slots.
 *
 * A job: fs; cur_slot, last_slot = the resident mCurrentFrame / mLastFrame; n = mCurrentFrame.N; nq = mLastFrame.N; last_ids[nq] =
 *   the pool id of mLastFrame.mvpMapPoints[i], -1 where it is NULL or mvbOutlier[i] (ORBmatcher.cc:1357-1360); velocity =
 *   mVelocity; last_Tcw = mLastFrame.mTcw as UpdateLastFrame left it (:857: that routine stays the caller's); K = fx, fy, cx, cy.
 * Call-wide: th (15 at :932 for the monocular case), min_matches (the reference's 20), check_ori (matcher's, :919),
 *   inv_level_sigma2, scale_factors and nlevels.  The image bounds are the frame set's.
 *
 * The rules, in the order they run:
 * 1. Pose (:925).  Tcw_pred = velocity * last_Tcw is gemm's small branch with len 4 and no C: element (r, c) is the four float
 *    products V[r][k] * T[k][c] summed left to right in float, then (float)((double)t * 1.0).  The product is made on the device.
 *    The frame's points are all NULL (:927): there are no base ids and no occupancy.
 * 2. Search 1 (:935 SearchByProjection(mCurrentFrame, mLastFrame, th, true)).  The projection is the pool's FRAME/FRAME gate set
 *    exactly as orbslamm_mappool.h states it, from Tcw_pred's Rcw and tcw: last_ids[i] < 0, or i at or above the last slot's device
 *    count: NO_POINT; invzc = (float)(1.0 / (double)z) with the division in double, invzc < 0: DEPTH; u, v outside the set's
 *    bounds: OUT_OF_IMAGE; the octave is the resident last frame's key's, radius = th * scale_factors[octave] (0 for an octave at
 *    or above nlevels: such a point finds nothing), the level window [octave - 1, octave + 1]; the bad flag is not consulted; qobs is the pool record's observed bit.  The search is the resident
 *    mode-4 search as orbw_track_frame_pose runs it: TH_HIGH 100, the rule of ORBmatcher.cc:1405-1407 (a feature matched by an
 *    observed point is occupied for the queries behind it), the query descriptor the resident last frame's row i as that search
 *    takes it, the rotation histogram under check_ori with the resident last frame's angles.  n_search[0] is nmatches behind the
 *    pruning (:1471): a feature two points took one after the other counts twice, as in the reference.
 * 3. Retry (:938-942).  Only when n_search[0] < min_matches does the search run again, from an all-NULL frame (:940), with
 *    2.0f * th: wide = 1 and n_search[1] is its count.  Otherwise wide = 0, n_search[1] = -1, the second pass does no search work
 *    for that job and the table that stands is the first's.
 * 4. Gate (:944).  The count that stands < min_matches: status ORBQ_MM_TOO_FEW.  No solve runs: track.opt is zero but for Tcw =
 *    Tcw_pred; ids_out[t] is the merge of the table that stands (the reference returns with those matches and the predicted pose in
 *    the frame), outlier_out[t] = 0, n_matches = that count, n_matches_map = 0.
 * 5. Solve and loop (:948-969).  Otherwise orbq_track_pose's path with discard = 1 over merged[t] = last_ids[assign[t]], from
 *    Tcw_pred: the edges in ASCENDING t, Xw the pool record's pos, the observation the resident mvKeysUn[t]; given the same edge
 *    list and pose the same bytes as orbq_track_pose (section 8s), n_matches / n_matches_map and the outlier byte convention (an
 *    outlier keeps its byte at 1 and gets ids_out[t] = -1) included.  Status ORBQ_MM_TRACKED.  The verdicts of :971-977
 *    (mbOnlyTracking: mbVO = nmatchesMap < 10, return nmatches > 20; else return nmatchesMap >= 10) are the caller's.
 * 6. Out, per job: the record; ids_out[j][n], outlier_out[j][n]; assign_out[j][n], where given: the last-frame feature matched to
 *    current feature t in the table that stands, or -1; status_out[j], where given: 2 * nq bytes, search 1's ORBW_ST_* bytes and
 *    then search 2's, ORBQ_MM_ST_NOT_RUN where search 2 did not run.
 * A feature at or above n takes no part (it is occupied for both searches).
 *
 * The call: synchronous, ONE synchronise, nine launches whatever n_jobs or the exits (stage, and twice: project, candidates,
 *   resolve, stage); one packed upload (job records | ids) and one copy down.  It runs on the handle's stream behind the slots'
 *   builds, in the handle's own scratch: no result set of the frame sets' track or BoW rings is taken or disturbed.  The pool's
 *   mutex is held from the checks to the synchronise, and the call leaves the reader event orbw_pool_set* wait for.  A job's bytes
 *   do not depend on its neighbours, the same call twice gives the same bytes, and jobs may name different frame sets of h, or the
 *   same slots twice.
 * Candidate arena: orbq_relocalize's rule.  A search whose candidates pass the job's share of the arena reports its need and the
 *   job stops; the host grows the arena to the largest need reported and runs the WHOLE call again (it has written nothing but its
 *   own scratch) -- at most three runs, search 1's need being settled by the second and search 2's by the third.  Partial results
 *   are never returned.  orbq_debug_motion_arena sets the share's starting size in entries, for tests (0: the default).
 * Refusals (never truncations; the argument checks come first and need no GPU):
 *   n_jobs == 0: ORBX_OK at once, nothing read or written.
 *   ORBX_E_UNSUPPORTED above ORBO_MAX_FRAMES jobs, n above ORBO_MAX_EDGES, more than ORBO_MAX_CALL_EDGES features a call, or jobs
 *   whose frame sets' caps add up to more than ORBO_MAX_CALL_EDGES.
 *   ORBX_E_INVALID for null arguments, n or nq negative or above the set's cap, a slot outside the set, a frame set of another
 *   handle, check_ori outside {0, 1}, min_matches < 0, th not finite or <= 0, nlevels outside [1, 16], an id outside the pool or
 *   never set; and, found by a kernel and reported behind it with the outputs unwritten: an edge's octave outside [0, nlevels), a
 *   feature with a point at or above the slot's device count.
 *   ORBX_E_CAPACITY when the arena still overflows in the third run.
 *   No CPU fallback. */
typedef struct {
    orbm_frameset_t* fs;
    int32_t cur_slot, last_slot;   /* resident mCurrentFrame / mLastFrame */
    int32_t n;                     /* mCurrentFrame.N */
    int32_t nq;                    /* mLastFrame.N */
    const int32_t* last_ids;       /* [nq] pool id of mLastFrame.mvpMapPoints[i]; -1: NULL or mvbOutlier[i] */
    float velocity[16];            /* mVelocity */
    float last_Tcw[16];            /* mLastFrame.mTcw as UpdateLastFrame left it (:857: the caller's) */
    float K[4];
} OrbqMotionJob;
#define ORBQ_MM_TRACKED 0
#define ORBQ_MM_TOO_FEW 1          /* :944 */
#define ORBQ_MM_ST_NOT_RUN 0xff
typedef struct { OrbqResult track; float Tcw_pred[16]; int32_t n_search[2]; int32_t wide; int32_t status; } OrbqMotionResult;
int orbq_track_motion_model(orbm_t* h, orbw_pool_t* pool, const OrbqMotionJob* jobs, int n_jobs, float th, int min_matches,
                            int check_ori, const float* inv_level_sigma2, const float* scale_factors, int nlevels,
                            OrbqMotionResult* out, int32_t* const* ids_out /* [n_jobs][n] */, uint8_t* const* outlier_out /* [n_jobs][n] */,
                            int32_t* const* assign_out /* may be null, or hold nulls: [n_jobs][n] */,
                            uint8_t* const* status_out /* may be null, or hold nulls: [n_jobs][2 nq] */);
/* for the tests of the overflow path: entries_per_job >= 0 sets the starting size of a job's share of the candidate arena (0: the
 * default; what the arena has grown to is dropped), -1 leaves it; last_runs, where given, gets how many times the last
 * orbq_track_motion_model on h ran its chain (1: no overflow; at most 3) */
int orbq_debug_motion_arena(orbm_t* h, int entries_per_job, int* last_runs);

#ifdef __cplusplus
}
#endif
#endif
