/* orbslamm_correct.h -- the loop-correction block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (orbu_store_t, the ORBX_* codes, the ORBR_ST_* statuses of orbslamm_refresh.h); including
 * either header gives both. */
#ifndef ORBSLAMM_CORRECT_H
#define ORBSLAMM_CORRECT_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * The correction of LoopClosing::CorrectLoop (src/LoopClosing.cc:455-524) and of its copy for map merging,
 * MultiMapper::UpdatePosesAndAdd (src/MultiMapper.cc:523-595), monocular, over a keyframe store and the map-point pool beside
 * it: the loop Sim3 propagated over K keyframes, every MapPoint they hold moved exactly once, UpdateNormalAndDepth of each
 * moved point, the keyframes' new poses and centres.  Line numbers below are LoopClosing.cc's unless a file is named.
 *
 * orbu_point_set_ref_kf(store, ids, kf_slots, n): mpRefKF of n pool ids as store slots, resident beside the pool in an int32
 *   array of the pool's size that the store owns (made at the first call, every id -1 until set).  ids[i] inside the pool;
 *   kf_slots[i] is -1 or in [0, kf_capacity); an id repeated within one call takes the LAST value.  A writer under the pool's
 *   concurrency rule, complete on return; argument checks (NULL, negative n) before the handle's.  n == 0: ORBX_OK at once.
 *   orbr_refresh_points does not read the array: its signature and behaviour are as they were.
 *
 * orbe_correct_sim3(store, slots, Tiw, K, anchor, Scw, skip_ids, n_skip, scale_factors, nlevels, commit, out_kf, out_pts,
 *   pts_cap, n_pts).  Synchronous, under the pool's mutex from the checks to the last synchronisation, a writer (it waits for
 *   the searches in flight) that steps the store's generation tag.  slots[K]: the keyframes of mvpCurrentConnectedKFs (:441-442)
 *   or mvpCurrentMapKFs as store slots; Tiw[12 i ..]: GetPose() of slots[i] as three float rows [R | t] (:459); anchor: the
 *   position in slots of mpCurrentKF / pKeyFrame; Scw: mg2oScw as 8 doubles, q in x y z w order, t[3], s (what
 *   orby_compute_sim3 returns); skip_ids[n_skip]: the pool ids that already carry mnCorrectedByKF == the anchor's mnId.
 *
 *   RULE 1, order.  CorrectedSim3 is a map<KeyFrame*, g2o::Sim3> walked in heap-address order (:480); the DEFINED CHOICE is
 *     ascending store slot, as in orbslamm_localmap.h, orbslamm_covis.h and orbslamm_refresh.h.  The RANK of a listed keyframe is
 *     its position in that order; the order of `slots` as given carries no meaning (a shuffled list gives the same bytes, out_kf
 *     following the caller's order), and the anchor stands wherever its slot falls.
 *   RULE 2, per keyframe, in binary64.  Twc of the anchor (:446 GetPoseInverse) as KeyFrame::SetPose forms it
 *     (src/KeyFrame.cc:99-106): Rwc = Rcw.t(), Ow = -Rwc*tcw in float (gemm, alpha = -1).  :463 Tic = Tiw*Twc: the 4x4 float
 *     product (gemm's small-matrix branch, four float products summed left to right).  :466 Sic = Sim3(toMatrix3d(Ric),
 *     toVector3d(tic), 1.0): the floats widened, Eigen's Quaterniond(R).  :467 CorrectedSiw = Sic * Scw by g2o's operator*
 *     (sim3.h:266-272: r = r*other.r, t = s*(r*other.t) + t, s = s*other.s), NO normalisation.  :445, :461 the anchor's
 *     CorrectedSiw is Scw itself, bit for bit.  :472-476 NonCorrected Siw = Sim3(toMatrix3d(Riw), toVector3d(tiw), 1.0).
 *     :512-518 the corrected pose: toRotationMatrix() of the un-normalised quaternion and t * (1. / s), both narrowed to float
 *     (Converter::toCvSE3).  :520 SetPose: the new centre Ow from that pose by the float arithmetic above.
 *   RULE 3, ownership.  :488 a keyframe holds the points of GetMapPointMatches(): every entry of its row that is not -1,
 *     ORBU_ENTRY_NO_VOTE entries included with bit 30 stripped.  :494 a point whose pool record carries ORBW_FLAG_BAD is skipped.
 *     :496 a point in skip_ids is skipped.  :480, :489 a point is OWNED by the lowest-ranked listed keyframe that holds it, at
 *     the lowest match-slot index of that row (mnCorrectedByKF keeps every later sighting out, :496, :506).  The keyframes' bad
 *     flags are not consulted: the reference does not consult them.
 *   RULE 4, move.  :500-505 P' = (float) CorrectedSwi.map(Siw.map((double) P)) with the owner's two Sim3; :484 inverse() as
 *     sim3.h:233-236 (r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s); map as sim3.h:144-146, s*(r*xyz) + t with
 *     QuaternionBase::_transformVector.
 *   RULE 5, UpdateNormalAndDepth inside the loop (:508).  The call for a point owned at rank r happens after SetPose (:520) of
 *     every listed keyframe of rank below r and before SetPose of rank r and of everything above.  The observations are the
 *     voting entries of the WHOLE store in ascending (slot, feature): orbslamm_refresh.h's definition and precondition.  Each
 *     observation reads its keyframe's centre so: the NEW centre when the keyframe is listed with rank < r, the store's present
 *     centre otherwise (the owner itself, higher ranks, keyframes outside the list); the reference keyframe's centre by the same
 *     rule.  CONSEQUENCE of rules 1 and 3 with that definition: a listed keyframe that observes the point holds it, so its rank
 *     is not below the owner's, and EVERY centre the rule reads is the store's present one; the new centres are not read before
 *     the commit writes them.  (tools/correct_ref.hpp runs the sequence and counts the observers that had been re-posed: none,
 *     in every scene of the tests.)  ref_kf is the resident array above.
 *     The arithmetic, the statuses (ORBR_ST_NO_OBSERVATION, ORBR_ST_NO_REF,
 *     ORBR_ST_LEVEL_RANGE, ORBR_ST_DONE; ORBR_ST_BAD cannot occur) and the ORBR_MAX_OBS refusal are the normal / depth half of
 *     orbslamm_refresh.h.  A point held only through ORBU_ENTRY_NO_VOTE slots has moved and reports ORBR_ST_NO_OBSERVATION.  A
 *     status other than ORBR_ST_DONE leaves normal and bounds as they were; the position moves regardless (:505 SetWorldPos has
 *     no gate).
 *   RULE 6, output and commit.  out_kf[i], in the CALLER's order: the corrected and the non-corrected Sim3 (8 doubles each, as
 *     Scw), the corrected Tiw[12], the new Ow[3], the count of points the keyframe owns.  out_pts[0 .. *n_pts): the moved points
 *     in the reference's visiting order, owner rank ascending and within an owner match-slot index ascending: id, owner slot
 *     (:507 mnCorrectedReference), owner index, the new position, normal / min / max as they stand after the call, n_obs, the
 *     status byte.  commit == 0 computes only.  Else ONE launch behind the check of the call's error word writes the positions,
 *     and the normal and bounds of the ORBR_ST_DONE points, into the pool, and the K new centres into the store.  Flags and
 *     descriptors are never touched.  The same call twice (commit == 0) gives the same bytes.
 *   REFUSALS, never truncations, with nothing written to the pool, the store or the outputs.  ORBX_E_INVALID: a NULL store,
 *     slots, Tiw, Scw, scale_factors, out_kf or n_pts, NULL skip_ids with n_skip > 0, NULL out_pts with pts_cap > 0; a negative
 *     K, n_skip or pts_cap; K == 0; anchor outside [0, K); a non-finite pose or Scw; s <= 0; nlevels outside [1, 16]; a listed
 *     slot that is unset, out of range or repeated; a skip id outside the pool or never set; a set keyframe without a centre or
 *     without octaves (as orbr_refresh_points).  ORBX_E_CAPACITY: more moved points than pts_cap, with the needed count in
 *     *n_pts (the one output written).  ORBX_E_UNSUPPORTED: a moved point above ORBR_MAX_OBS observations.  The argument checks
 *     come before the handle's and need no GPU.
 * Scratch grows only; no allocation after the first call of a size.  No CPU fallback. */
typedef struct {
    double corrected[8];       /* CorrectedSim3[pKFi]: q x y z w, t[3], s */
    double non_corrected[8];   /* NonCorrectedSim3[pKFi] */
    float Tiw[12];             /* correctedTiw, rows [R | t] */
    float Ow[3];               /* GetCameraCenter() after SetPose(correctedTiw) */
    int32_t n_points;          /* the moved points whose mnCorrectedReference is this keyframe */
} OrbeKeyFrame;
typedef struct {
    int32_t id;                /* pool id */
    int32_t owner_slot;        /* mnCorrectedReference */
    int32_t owner_idx;         /* the match slot of the owner through which the point was reached */
    float pos[3], normal[3];
    float min_distance, max_distance;
    int32_t n_obs;
    uint8_t status;            /* ORBR_ST_* of UpdateNormalAndDepth */
    uint8_t pad[3];
} OrbePoint;
int orbu_point_set_ref_kf(orbu_store_t* store, const int32_t* ids, const int32_t* kf_slots, int n);
int orbe_correct_sim3(orbu_store_t* store, const int32_t* slots, const float* Tiw /* [12 K] */, int K, int anchor, const double* Scw /* [8] */,
                      const int32_t* skip_ids, int n_skip, const float* scale_factors, int nlevels, int commit, OrbeKeyFrame* out_kf /* [K] */,
                      OrbePoint* out_pts /* [pts_cap] */, int pts_cap, int* n_pts);

#ifdef __cplusplus
}
#endif
#endif
