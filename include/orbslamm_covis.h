/* orbslamm_covis.h -- the covisibility block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (orbu_store_t, the ORBX_* codes); including either header gives both. */
#ifndef ORBSLAMM_COVIS_H
#define ORBSLAMM_COVIS_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * KeyFrame::UpdateConnections' counting and ordering (src/KeyFrame.cc:300-400) and the body of LocalMapping::KeyFrameCulling's
 * outer loop (src/LocalMapping.cc:632-698, monocular), for K target keyframes in one call, over a keyframe store and its pool
 * (orbslamm_localmap.h).  Integers only.
 *
 * Terms (those of orbu_update_local_map's vote):
 *   an OBSERVATION of pool id p   a voting entry (j, i): keyframe slot j is set, entries[j][i] == p, bit 30
 *                                 (ORBU_ENTRY_NO_VOTE) clear.  Every voting entry counts: a keyframe that holds p at two voting
 *                                 features contributes two.  A keyframe's own bad flag is not consulted (a bad keyframe's
 *                                 entries are NO_VOTE already: SetBadFlag erased it from its points).
 *   Observations(p)               the number of its observations.
 *   a POINT OF KEYFRAME k         a match slot: a non-empty entry of k, bit 30 masked off, NO_VOTE or not, whose pool record
 *                                 carries no ORBW_FLAG_BAD; taken once per slot it fills.
 *
 * orbu_kf_set_octaves(store, slot, octaves, n): mvKeysUn[i].octave as one byte per feature of a SET keyframe; n <= stride, the
 *   bytes behind n become 0.  The block (kf_capacity x stride bytes) is allocated at the first call; a store that never calls
 *   it allocates nothing.  Octaves persist across later orbu_kf_set* calls on the slot.  NULL octaves or n < 0, a slot that is
 *   unset or out of range: ORBX_E_INVALID; n > stride: ORBX_E_UNSUPPORTED; more than ORBN_MAX_OCTAVE_VALUES distinct byte
 *   values over the life of the store: ORBX_E_UNSUPPORTED, nothing written.  Complete on return.
 *
 * orbn_update_connections(store, targets, K, th, &result): targets[K] set slots (else ORBX_E_INVALID), repeats allowed,
 *   0 <= K <= ORBU_MAX_KEYFRAMES (above: ORBX_E_UNSUPPORTED), th >= 0 the reference's 15.  Per target k:
 *     counter   for every point p of k and every observation (j, i) of p with j != k (slot inequality): counter[j]++ (:313-331).
 *               cnt row = the (kf, weight) with weight > 0 in ASCENDING kf: mConnectedKeyFrameWeights, below th included.
 *     empty     status ORBN_EMPTY, both rows empty, kf_max -1, n_max 0 (:334 returns, the old connections stay).
 *     maximum   n_max / kf_max: strict > in ascending slot (:345-351) = the LOWEST slot among the largest weights.
 *     ordered   the (kf, weight) with weight >= th, or the single (kf_max, n_max) when there are none (:352-363), as sort on
 *               pair<int,KeyFrame*> and push_front leave them (:365-372): weight DESCENDING, among equal weights slot
 *               DESCENDING.  The members with weight >= th are the keyframes whose AddConnection(this, w) the caller replays.
 *     DEFINED CHOICES: the reference iterates map<KeyFrame*,int> and compares KeyFrame* in heap-address order; here both
 *     are slot order, as in orbslamm_localmap.h.
 *   A target's rows are the same bytes alone, in any batch, at any position.  The store's graph record is NOT written.
 *
 * orbn_culling_counts(store, targets, K, th_obs, &result): th_obs >= 0 the reference's 3.  Per target k, for every point p of
 *   k at feature i: n_mps++ (:666); when Observations(p) > th_obs (:667) the observations (j, i') of p with j != k and
 *   octave[j][i'] <= octave[k][i] + 1 (as ints, :679) are counted, and when there are >= th_obs (:686): n_redundant++.
 *   redundant[k] = (double)n_redundant > 0.9 * (double)n_mps (:695), computed on the host.  ORBX_E_INVALID unless every set
 *   keyframe of the store has octaves.  The stereo depth gate (:660-664) is not there.
 *
 * Both: synchronous, under the pool's mutex, after the pool's readers; the result's pointers are views into blocks the
 * store owns, valid until the store's next call; blocks grow only.  A refusal leaves *result as it was.  K == 0 returns
 * ORBX_OK at once.  Argument checks come before the handle's and need no GPU.  No CPU fallback. */
#define ORBN_OK 0
#define ORBN_EMPTY 1
#define ORBN_MAX_OCTAVE_VALUES 16
typedef struct {
    int32_t K;
    const int32_t* status;     /* [K] ORBN_OK | ORBN_EMPTY */
    const int32_t* kf_max;     /* [K] */
    const int32_t* n_max;      /* [K] */
    const int32_t* cnt_start;  /* [K + 1] */
    const int32_t* cnt_kf;     /* [cnt_start[K]] */
    const int32_t* cnt_w;
    const int32_t* ord_start;  /* [K + 1] */
    const int32_t* ord_kf;     /* [ord_start[K]] */
    const int32_t* ord_w;
} OrbnConnections;
typedef struct {
    int32_t K;
    const int32_t* n_mps;        /* [K] */
    const int32_t* n_redundant;  /* [K] */
    const uint8_t* redundant;    /* [K] */
} OrbnCulling;
int orbu_kf_set_octaves(orbu_store_t* store, int slot, const uint8_t* octaves, int n);
int orbn_update_connections(orbu_store_t* store, const int32_t* targets, int K, int th, OrbnConnections* result);
int orbn_culling_counts(orbu_store_t* store, const int32_t* targets, int K, int th_obs, OrbnCulling* result);

#ifdef __cplusplus
}
#endif
#endif
