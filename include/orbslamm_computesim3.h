/* orbslamm_computesim3.h -- the block of liborbslamm_hip.so's C ABI that closes LoopClosing::ComputeSim3's chain behind the
 * Sim3Solver on the device: ORBmatcher::SearchBySim3 and Optimizer::OptimizeSim3 for any number of
 * (current keyframe, candidate keyframe, Sim3) jobs in ONE call.  Included by orbslamm_hip.h, whose types it uses (orbm_t,
 * orbm_frameset_t, orbw_pool_t, orbu_store_t, OrbzProblem, OrbzResult, the ORBX_* codes); including either gives both. */
#ifndef ORBSLAMM_COMPUTESIM3_H
#define ORBSLAMM_COMPUTESIM3_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * LoopClosing::ComputeSim3 (src/LoopClosing.cc:296-347) and MultiMapper::Run, per candidate behind Sim3Solver::iterate:
 * SearchBySim3(pKF1, pKF2, vpMatches12, s, R, t, 7.5) (src/ORBmatcher.cc:1104-1328, monocular), then OptimizeSim3(pKF1, pKF2,
 * vpMatches12, gScm, 10, mbFixScale) (src/Optimizer.cc:1348-1543).  Everything the two read is resident: the points in the pool,
 * the two keyframes' match lists in the keyframe store, their mvKeysUn, descriptors and grid in two slots of a frame set.  One
 * packed upload (the job records and the entering match arrays), a number of launches that does not depend on the number of jobs,
 * one copy down, one synchronise; no atomics; nothing per map point or per correspondence goes up.
 *
 * A job: fs, slot1, slot2: the two keyframes as slots of one resident frame set; kf1, kf2: their slots in the keyframe store
 *   (entries[kf][q] = pool id of GetMapPointMatches()[q], bit 30 = ORBU_ENTRY_NO_VOTE aside, or -1); n1, n2 = N1, N2; prob exactly
 *   as orbz_optimize_sim3 takes it; R12, t12, s12 what the reference hands SearchBySim3 (:1104); bounds1, bounds2 = mnMinX,
 *   mnMaxX, mnMinY, mnMaxY of pKF1 and pKF2; th (7.5 in both callers); m12_id[i] the pool id of vpMatches12[i] as it enters (the
 *   solver's inliers, LoopClosing.cc:319-324) or -1, m12_idx2[i] that point's GetIndexInKeyFrame(pKF2) or -1 (n1 ints each; both
 *   may be null: no entering match).
 * Per call, shared by its jobs as in OptimizeSim3T::RunAll: the two keyframes' mvScaleFactors, their orbl_level_breaks tables
 *   (nlevels + 1 floats), their mvInvLevelSigma2, and nlevels.
 *
 * 1. Marks (:1131-1144): already1[i] = m12_id[i] >= 0; already2[m12_idx2[i]] = 1 where m12_id[i] >= 0 and 0 <= m12_idx2[i] <
 *    n2.  Several i may name one idx2: they write the same byte.
 * 2. Pass 1->2 (:1150-1227): every i1 < n1 whose entry e = entries[kf1][i1] is not -1 (:1154 !pMP), is not marked (:1154) and
 *    whose pool record e & ~ORBU_ENTRY_NO_VOTE carries no ORBW_FLAG_BAD (:1157).  orbq_track_reference's validity rule: an entry
 *    with ORBU_ENTRY_NO_VOTE takes part, a feature at or above the store's stride holds no point.  In float, in this order (the
 *    adapter's cvsem restatement, include/ORBmatcher_hip.hpp:814-826): pf = R1w Xw + t1w (:1161); pt = sR21 pf + t21 (:1162)
 *    with sR21 = (1.0 / s12) R12^T and t21 = -sR21 t12 (:1122-1123) formed on the host; skipped on pt.z < 0.0 (:1165); invz =
 *    (float)(1.0 / (double)z) (:1168); u = fx x + cx, v = fy y + cy with pKF1's intrinsics IN BOTH DIRECTIONS (:1107-1110,
 *    sic); pKF2's IsInImage (:1176: >= min, < max); dist3D = norm(pt) inside [0.8f min, 1.2f max] of the pool record's raw
 *    bounds (:1179-1185); the level from pKF2's break table with ratio = max / dist3D (:1188); a level outside [0, nlevels)
 *    skips the point (the adapter's defined rule, ORBmatcher_hip.hpp:825; the reference indexes mvScaleFactors with it); radius
 *    th sf2[level] (:1191), GetFeaturesInArea over slot2's grid (:1193), the octave gate [level - 1, level] (:1209), strict <
 *    so the first wins (:1216), taken when bestDist <= TH_HIGH = 100 (:1223).  No viewing-angle gate, no chi-square test.
 * 3. Pass 2->1 (:1230-1307): the mirror with sR12 = s12 R12 and t12 (:1121), pKF2's points not marked in already2, into slot1
 *    with pKF1's bounds, break table and scale factors.
 * 4. Agreement (:1309-1325), ascending i1: vnMatch1[i1] = idx2 >= 0 and vnMatch2[idx2] == i1 make vpMatches12[i1] the point of
 *    pKF2's feature idx2, a NEW match; n_found counts them (SearchBySim3's return value: new matches only).
 * 5. Walk (Optimizer.cc:1401-1440), ascending i over the entering and the new matches: pMP1 = entries[kf1][i], null skips
 *    (:1419); pMP2 and i2 of an entering match are m12_id[i] and m12_idx2[i]; of a new match pMP2 = entries[kf2][idx2] with bit
 *    30 cleared and i2 = idx2 -- unless the entry carries ORBU_ENTRY_NO_VOTE: then i2 = -1, the point's observations do not
 *    list the keyframe.  Either point bad in the pool, or i2 < 0, skips (:1421); the match stays in the table.
 *    DEFINED PRECONDITION: a voting entry at slot q of a keyframe's row means GetIndexInKeyFrame(that keyframe) == q (the store
 *    invariant the covisibility entries rely on).
 *    The correspondences are compacted in order; the gather is mvKeysUn[i] of slot1, mvKeysUn[i2] of slot2, X1w / X2w from the pool.
 * 6. Solve (:1484-1541): orbz_optimize_sim3's own (section 8p).  Given the same correspondence list it returns the same
 *    OrbzResult, and removed_out[j][c] is orbz_optimize_sim3's byte of correspondence c (n1 bytes are written: n_corr of them, then
 *    zeros).
 * 7. Out, per job: opt; n_found; n_corr.  match_out[j][i] = the pKF2 feature index of vpMatches12[i] as OptimizeSim3 leaves
 *    it (an entering match: m12_idx2[i]; -1 where there is none or either check nulled it, :1497, :1532); ids_out[j][i] the
 *    pool id of that point, or -1.  The early return of :1514 leaves the Sim3 as it came (written = 0, n_in = 0), the matches
 *    nulled by the first check stay nulled.  A job with fewer than 3 correspondences still runs (zero: as orbz_optimize_sim3
 *    returns it).  The verdict nInliers >= 20 (LoopClosing.cc:333) is the caller's.
 *    Optional (null, or nulls inside): status_out[j], n1 + n2 bytes, one per (direction, feature), pass 1->2's first: the gate
 *    that ended the feature (ORBY_ST_*); vnmatch_out[j], n1 + n2 ints: vnMatch1 | vnMatch2 as the two passes left them (a debug
 *    copy-down for the tests).
 * Synchronous.  Jobs may name different frame sets of the handle h, and the same keyframe any number of times; a job's bytes do
 *   not depend on its neighbours and the same call twice gives the same bytes.  The pool's mutex (the store shares it) is held
 *   from the checks to the synchronise and the call leaves the reader event orbw_pool_set* and orbu_kf_set* wait for.
 * Refusals (never truncations; the argument checks come first and need no GPU):
 *   n_jobs == 0: ORBX_OK at once.
 *   ORBX_E_UNSUPPORTED above ORBZ_MAX_PROBLEMS jobs, n1 or n2 above ORBZ_MAX_CORR, more than ORBZ_MAX_CALL_CORR features (n1 + n2
 *   over the jobs) a call.
 *   ORBX_E_INVALID for null arguments, negative counts or slots, n1 or n2 above the set's cap, a slot outside the set, a frame
 *   set of another handle, a store of another pool, kf1 or kf2 outside the store or not set, an m12_id outside the pool or never
 *   set, an m12_idx2 >= n2 or below -1 (-1 beside a point is taken: that match stays and gets no edge, as the reference's
 *   i2 < 0), nlevels outside [1, 16], a break table that does not ascend, only one of m12_id and m12_idx2, a th2, th or s12 that
 *   is not finite or not positive; and, found by the kernel and reported behind it with the outputs unwritten: an edge's octave
 *   outside [0, nlevels), a matched feature at or above its slot's device count, or a match of a pass at or above the job's n of
 *   the keyframe searched.
 *   No CPU fallback. */
typedef struct {
    orbm_frameset_t* fs; int32_t slot1, slot2;
    int32_t kf1, kf2;
    int32_t n1, n2;
    OrbzProblem prob;
    float R12[9], t12[3], s12;
    float bounds1[4], bounds2[4];
    float th;
    const int32_t* m12_id;
    const int32_t* m12_idx2;
} OrbyJob;
typedef struct { OrbzResult opt; int32_t n_found, n_corr; } OrbyResult;
/* the status byte of a (direction, feature) */
#define ORBY_ST_NO_POINT 0        /* a null entry, or a feature at or above the store's stride */
#define ORBY_ST_MARKED 1          /* already matched as the call entered */
#define ORBY_ST_BAD 2             /* the pool record carries ORBW_FLAG_BAD */
#define ORBY_ST_DEPTH 3
#define ORBY_ST_OUTSIDE_IMAGE 4
#define ORBY_ST_DISTANCE 5
#define ORBY_ST_LEVEL_RANGE 6
#define ORBY_ST_NO_CANDIDATE 7    /* no feature in the window and the octave gate, or the best above TH_HIGH */
#define ORBY_ST_FOUND 8
int orby_compute_sim3(orbm_t* h, orbw_pool_t* pool, orbu_store_t* store, const OrbyJob* jobs, int n_jobs,
                      const float* scale_factors1, const float* scale_factors2, const float* level_breaks1, const float* level_breaks2,
                      const float* inv_level_sigma2_1, const float* inv_level_sigma2_2, int nlevels, OrbyResult* out,
                      int32_t* const* match_out /* [n_jobs][n1] */, int32_t* const* ids_out /* [n_jobs][n1] */,
                      uint8_t* const* removed_out /* [n_jobs][n1]; may be null, or hold nulls */,
                      uint8_t* const* status_out /* [n_jobs][n1 + n2]; may be null, or hold nulls */,
                      int32_t* const* vnmatch_out /* [n_jobs][n1 + n2]; may be null, or hold nulls */);

#ifdef __cplusplus
}
#endif
#endif
