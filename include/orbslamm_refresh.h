/* orbslamm_refresh.h -- the map-point refresh block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (orbu_store_t, orbw_pool_t, OrbwPoint, orbm_frameset_t, the ORBX_* codes); including
 * either header gives both. */
#ifndef ORBSLAMM_REFRESH_H
#define ORBSLAMM_REFRESH_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and MapPoint::UpdateNormalAndDepth (:330-371), monocular,
 * for n points of a map-point pool in one call, over the keyframe store beside it (orbslamm_localmap.h, orbslamm_covis.h):
 * the pool's records are refreshed IN PLACE from the store's observations, so that after a bundle adjustment 12 bytes of
 * position a point go up instead of a 68-byte record computed on the host.
 *
 * What the store holds for it (setters; each a writer under the pool's concurrency rule, complete on return, argument checks
 * before the handle's).  A store that never calls them allocates nothing:
 *   orbu_kf_set_descriptors(store, slot, desc, n)        mDescriptors of a SET keyframe, n x 32 bytes from the host; n <= stride
 *     (above: ORBX_E_UNSUPPORTED), the rows behind n become zero.  The block (kf_capacity x pitch x 32 bytes, the pitch the
 *     stride rounded up to 4) is made at the first call of either descriptor setter and persists across orbu_kf_set*.
 *   orbu_kf_set_descriptors_frame(store, slot, fs, fs_slot)   the same bytes device to device from slot fs_slot of a frame
 *     set; the count is the slot's device count (above the stride: ORBX_E_UNSUPPORTED).  The frame set and the pool must be
 *     on one matcher handle (else ORBX_E_INVALID).
 *   orbu_kf_set_centres(store, slots, Ow, n)             GetCameraCenter() of n SET keyframes, three floats each; a slot
 *     repeated within one call takes the LAST value.
 *   Octaves: orbu_kf_set_octaves (orbslamm_covis.h), unchanged.
 *   NULL pointers, a negative n, a slot that is unset or out of range: ORBX_E_INVALID.
 * orbw_debug_pool_get(pool, ids, n, out): the pool's records of n SET ids copied down (a reader that synchronises), so that
 *   the tests see what a commit wrote.
 *
 * orbr_refresh_points(store, ids, ref_kf, new_pos, n, what, scale_factors, nlevels, commit, out).  Synchronous, under the
 *   pool's mutex from the checks to the last synchronisation, a writer (it waits for the searches in flight) that steps the
 *   store's generation tag.  ids[i]: a set pool id, no id twice.  ref_kf[i]: the store slot of mpRefKF, or -1.  new_pos
 *   (3 n floats or NULL): SetWorldPos in front of the refresh (Optimizer.cc:798-799, LoopClosing.cc:508-511); when given,
 *   every step reads new_pos[3 i ..] as point i's position.  what: ORBR_DESCRIPTOR | ORBR_NORMAL_DEPTH.
 *   OBSERVATIONS (the terms of orbslamm_covis.h): an observation of p is a voting entry (j, q): slot j set, entries[j][q] == p,
 *     bit 30 clear; a point's list is taken in ASCENDING (j, q) -- the DEFINED CHOICE for map<KeyFrame*,size_t>'s heap-address
 *     order.  Defined precondition: a point has at most one voting entry per keyframe; where violated every voting entry is an
 *     observation, in that order, and the reference keyframe's feature is its lowest q.
 *   ORBR_DESCRIPTOR: the pool record bad -> ORBR_ST_BAD (:251); no observation -> ORBR_ST_NO_OBSERVATION (:256); the descriptors
 *     are desc[j][q] of the observations whose keyframe is not ORBU_KF_BAD (:265), in order; none -> ORBR_ST_ALL_KF_BAD (:269).
 *     With N of them: row i = the N Hamming distances d(i, .), the 0 to itself included; its median = the element of 0-based
 *     rank (N - 1) / 2 (integer division) of the sorted row (:294); the winner is the first i with the strictly smallest
 *     median (:296).  Integers in [0, 256]: nothing rounds.
 *   ORBR_NORMAL_DEPTH: BAD and NO_OBSERVATION as above (:338, :345).  Over ALL observations in order, bad keyframes included
 *     (:350): normali = P - Ow[j] in float, nd = cv::norm (double sum of squares, sqrt), a = (float)(1. / nd), normal[c] =
 *     normali[c] * a + normal[c] from zeros (one float product, one float sum, no contraction); at the end normal[c] =
 *     (float)((double)normal[c] * (1. / n)), or normal[c] + 0.f when n == 1.  A zero nd gives what the arithmetic gives.
 *     ref_kf[i] == -1 or a slot that is not among the observations -> ORBR_ST_NO_REF (the reference would insert a zero index
 *     into its copy of the map: the DEFINED replacement); level = octave[ref][q_ref] outside [0, nlevels) -> ORBR_ST_LEVEL_RANGE
 *     (the reference indexes mvScaleFactors out of bounds); else dist = (float)cv::norm(P - Ow[ref]), max = dist * sf[level],
 *     min = max / sf[nlevels - 1].
 *   A status other than ORBR_ST_DONE leaves the three fields of that half as they were; a half not asked for reports
 *     ORBR_ST_NOT_ASKED.
 *   OUT, per point: the record as it stands after the call (pos = new_pos[i] when given; the pool's own values where a half
 *     did not run), n_obs (the observations) and n_desc (those whose keyframe is not bad), both whatever `what` and the
 *     statuses are; best_kf / best_idx (the winner's slot and feature), -1 unless the descriptor half is DONE; the two status
 *     bytes.  A point's bytes are the same alone, in any batch, at any position; the same call twice gives the same bytes.
 *   COMMIT: 0 computes only.  Else normal / min / max and desc of the halves that are DONE are written into the pool's
 *     arrays in place, and with new_pos the position of EVERY listed id (SetWorldPos has no gate).  The flags byte is never
 *     touched.  The commit is a launch of its own behind the check of the call's error word: a call refused after its
 *     kernels ran has written nothing, neither to the pool nor to out.
 *   REFUSALS, never truncations.  n == 0: ORBX_OK at once.  ORBX_E_INVALID: a NULL store, ids, ref_kf, scale_factors or out; a
 *     negative n; what zero or with unknown bits; nlevels outside [1, 16]; a non-finite new_pos; an id outside the pool, never
 *     set, or repeated; a ref_kf that is neither -1 nor a set slot; with ORBR_DESCRIPTOR a set keyframe without descriptors;
 *     with ORBR_NORMAL_DEPTH a set keyframe without a centre or without octaves.  ORBX_E_UNSUPPORTED: n above the pool's
 *     capacity; a listed point with more than ORBR_MAX_OBS observations (found on the device once the index is counted).
 * Scratch grows only; no allocation after the first call of a size.  No CPU fallback. */
#define ORBR_DESCRIPTOR 1
#define ORBR_NORMAL_DEPTH 2
#define ORBR_MAX_OBS 1024
#define ORBR_ST_NOT_ASKED 0
#define ORBR_ST_DONE 1
#define ORBR_ST_BAD 2             /* the pool record carries ORBW_FLAG_BAD */
#define ORBR_ST_NO_OBSERVATION 3
#define ORBR_ST_ALL_KF_BAD 4      /* descriptor half: every observing keyframe is bad */
#define ORBR_ST_NO_REF 5          /* normal / depth half: ref_kf -1 or not observing */
#define ORBR_ST_LEVEL_RANGE 6     /* normal / depth half: the reference octave outside [0, nlevels) */
typedef struct {
    float pos[3], normal[3];
    float min_distance, max_distance;
    uint8_t desc[32];
    int32_t n_obs, n_desc;
    int32_t best_kf, best_idx;
    uint8_t st_descriptor, st_normal_depth;
    uint8_t pad[2];
} OrbrPoint;
int orbu_kf_set_descriptors(orbu_store_t* store, int slot, const uint8_t* desc, int n);
int orbu_kf_set_descriptors_frame(orbu_store_t* store, int slot, orbm_frameset_t* fs, int fs_slot);
int orbu_kf_set_centres(orbu_store_t* store, const int32_t* slots, const float* Ow, int n);
int orbw_debug_pool_get(orbw_pool_t* pool, const int32_t* ids, int n, OrbwPoint* out);
int orbr_refresh_points(orbu_store_t* store, const int32_t* ids, const int32_t* ref_kf, const float* new_pos /* [3 n] or NULL */,
                        int n, int what /* ORBR_DESCRIPTOR | ORBR_NORMAL_DEPTH */, const float* scale_factors, int nlevels,
                        int commit, OrbrPoint* out /* [n] */);

#ifdef __cplusplus
}
#endif
#endif
