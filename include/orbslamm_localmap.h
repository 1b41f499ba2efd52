/* orbslamm_localmap.h -- the local-map block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (orbw_pool_t, orbm_frameset_t, OrbmProjParams, OrbwView, the ORBX_* codes); including
 * either header gives both. */
#ifndef ORBSLAMM_LOCALMAP_H
#define ORBSLAMM_LOCALMAP_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * Tracking::UpdateLocalMap (src/Tracking.cc:1253-1261): UpdateLocalKeyFrames (:1289-1397) and UpdateLocalPoints
 * (:1263-1286), from keyframes that LIVE in HBM beside a map-point pool.  Per frame the frame's own <= n pool ids go up; the
 * local keyframe list, mvpLocalMapPoints (L), the byte "already in this frame" per element (seen) and the count of the list
 * SearchLocalPoints searches (S = L without the seen ones) come down; S stays on the device, where
 * orbw_track_local_map_resident reads it.  Integers only: no floating point anywhere.
 *
 * The store.  orbu_store_create(pool, kf_capacity, stride, max_children, max_local_points): kf_capacity keyframe slots, none
 *   set, beside ONE pool whose mutex it shares (LocalMapping's thread may update while Tracking's thread queries).  Every
 *   entry below is synchronous and holds that mutex for its duration.  kf_capacity in [1, ORBU_MAX_KEYFRAMES], stride in
 *   [1, ORBU_MAX_STRIDE], max_children in [0, ORBU_MAX_CHILDREN], max_local_points in [1, ORBW_POOL_MAX_CAPACITY]; above:
 *   ORBX_E_UNSUPPORTED; below: ORBX_E_INVALID.  Destroy the store before its pool.
 *   Per keyframe slot k:
 *     entries[stride]  GetMapPointMatches() as pool ids; -1: an empty slot.  Bit 30 set (ORBU_ENTRY_NO_VOTE, free because pool
 *                      ids are < 2^22) marks a point that sits in the keyframe's match slot while the point's observations do
 *                      not list the keyframe (!pMP->IsInKeyFrame(pKF)): every keyframe between CreateNewKeyFrame and
 *                      ProcessNewKeyFrame.  Such an entry feeds the point list (:1270 walks the match slots) and casts no vote
 *                      (:1300 walks the observations).
 *     flags            bit 0 isBad() (ORBU_KF_BAD), bit 1 "set" (ORBU_KF_SET; the store keeps it, a caller's bit 1 is ignored).
 *     graph            up to ORBU_MAX_NEIGHBOURS slots in mvpOrderedConnectedKeyFrames order (GetBestCovisibilityKeyFrames(10);
 *                      -1: none, skipped), the parent slot or -1, up to max_children children.
 *   An unset slot that a graph record names is a keyframe with no entries that is not bad.
 * DEFINED CHOICES, where the reference iterates map<KeyFrame*,int> and set<KeyFrame*> in heap-address order:
 *   - the voted keyframes are taken in ASCENDING SLOT (so kf_max is the lowest slot among those with the most votes);
 *   - the children are taken in the order the caller gives.
 *   The drop-in (include/Tracking_hip.hpp) uses slot = mnId and children ascending by mnId.
 *
 * Setters.  OrbuKeyFrames is nkf records as arrays: slot[i], flags[i], n[i] entries (concatenated in `entries`), neigh[10 i ..],
 *   parent[i], nchildren[i] children (concatenated in `children`).  orbu_kf_set writes whole records (entries behind n[i] become
 *   -1); orbu_kf_set_graph the graph records alone and orbu_kf_set_flags the flags alone, of keyframes that are set;
 *   orbu_kf_set_entries single match slots idx[] / vals[] of one set keyframe (AddMapPoint / EraseMapPointMatch / Replace).
 *   Each returns with the update COMPLETE on the device.  Every id is validated on the host before any launch: a pool id
 *   (bit 30 aside) must be set in the pool at that time -- pool slots never become unset, so a device-made list never names
 *   an unset slot --, a keyframe slot must lie in [0, kf_capacity): else ORBX_E_INVALID.  n[i] > stride, an idx >= stride or
 *   nchildren[i] > max_children: ORBX_E_UNSUPPORTED.  A keyframe (an index) repeated within one call takes the LAST value.
 *   Argument checks come before the handle's and need no GPU; a count of 0 returns ORBX_OK at once.
 *
 * orbu_update_local_map(store, frame_ids, n, max_keyframes, &result): frame_ids[i] is the pool id of
 *   mCurrentFrame.mvpMapPoints[i] or -1 (anything else that is not a set pool id: ORBX_E_INVALID; n > ORBU_MAX_FRAME_POINTS:
 *   ORBX_E_UNSUPPORTED); max_keyframes >= 0 is the reference's 80.
 *   1 stamp   every frame id whose pool record is not bad counts once per feature it fills (a point in two features votes
 *             twice, as keyframeCounter[..]++ at :1302 does).
 *   2 vote    votes[k], k set = the sum over k's entries that are neither empty nor NO_VOTE of the point's count.  Bad
 *             keyframes are counted too (:1302 does not look).
 *   3 select  no vote at all: status ORBU_NO_VOTES, nothing else written (:1311 returns, the old lists stay).  Else the voted
 *             keyframes that are not bad, ascending (:1321-1336); kf_max the first with strictly the most votes, -1 when all
 *             are bad (the list is then empty).  The expansion (:1340-1390) walks THAT GROUP ONLY (the end iterator is taken
 *             before the loop); each step: stop when size() > max_keyframes (:1343); the first of the <= 10 neighbours that
 *             is neither bad nor included (:1350-1362); the first such child (:1365-1377); the parent when not included --
 *             NOT tested for bad -- and then the `break` of :1386 leaves the OUTER loop: the expansion ends there.
 *   4 points  :1263-1286 over the list: in (list position, entry index) order the first sighting of every pool id whose record
 *             is not bad; NO_VOTE entries count.  seen[i] = 1 when L[i] was stamped in step 1: the points SearchLocalPoints
 *             skips at :1228.  S = L without them, in order.  |L| > max_local_points: ORBX_E_CAPACITY, result->nL holds the
 *             needed count, no list is returned and the store has no completed update.
 *   The result's pointers are views into the store's pinned block, valid until the store's next call.
 * orbu_local_points(store, kf_list, nkf, frame_ids, n, &result): steps 1 and 4 alone over the caller's list (slots in [0,
 *   kf_capacity), nkf <= kf_capacity, repeats allowed): what follows ORBU_NO_VOTES, where the reference still runs
 *   UpdateLocalPoints over the old list.  status ORBU_OK, kf_max -1, kf = the list as given, votes NULL.
 * orbu_debug_set_generation: the generation tag of the pool-sized scratch (tests force the wrap: the call that finds the tag
 *   at 0xffffffff clears the scratch once and starts over at 1).  The tag only moves forward: a smaller one is ORBX_E_INVALID.
 *
 * orbu_debug_resident_list: the device-resident S of the last completed update copied down (n = nS; a smaller buffer:
 *   ORBX_E_CAPACITY), so that the tests see the array the resident search reads and not only what the host can derive.
 *
 * orbw_track_local_map_resident: orbw_track_local_map with ids = the store's device-resident S and nq = the nS of the
 *   store's last completed update; nothing per point goes up.  assign[t] is the position in S.  orbw_track_status, the
 *   overflow replay and the ceilings are orbw_track_local_map's.  ORBX_E_INVALID when the store has no completed update or
 *   belongs to another pool.  The store's next update waits for the projection kernel of every search in flight.
 *   ONE THREAD makes a store's per-frame calls (orbu_update_local_map / orbu_local_points and the resident search): the search
 *   takes nS under the mutex and launches after releasing it, so another thread's update in between would leave the count and
 *   the list of different updates (ids still in bounds, but not one frame's list).  The setters may come from any thread.
 * No CPU fallback.  Blocks grow only; no allocation after the first call of a size. */
#define ORBU_ENTRY_NO_VOTE (1 << 30)
#define ORBU_KF_BAD 1
#define ORBU_KF_SET 2
#define ORBU_MAX_NEIGHBOURS 10
#define ORBU_MAX_KEYFRAMES (1 << 17)
#define ORBU_MAX_STRIDE (1 << 13)
#define ORBU_MAX_CHILDREN 1024
#define ORBU_MAX_FRAME_POINTS (1 << 20)
#define ORBU_OK 0
#define ORBU_NO_VOTES 1
typedef struct {
    int32_t nkf;
    const int32_t* slot;      /* [nkf] */
    const uint8_t* flags;     /* [nkf] */
    const int32_t* n;         /* [nkf] */
    const int32_t* entries;   /* [sum n] */
    const int32_t* neigh;     /* [10 nkf] */
    const int32_t* parent;    /* [nkf] */
    const int32_t* nchildren; /* [nkf] */
    const int32_t* children;  /* [sum nchildren] */
} OrbuKeyFrames;
typedef struct {
    int32_t status;           /* ORBU_OK | ORBU_NO_VOTES */
    int32_t kf_max;
    int32_t nkf;
    int32_t nL, nS;
    const int32_t* kf;        /* [nkf] */
    const int32_t* L;         /* [nL] */
    const uint8_t* seen;      /* [nL] */
    const int32_t* votes;     /* [kf_capacity] (0 for unset slots), or NULL */
} OrbuResult;
typedef struct orbu_store orbu_store_t;
int orbu_store_create(orbw_pool_t* pool, int kf_capacity, int stride, int max_children, int max_local_points, orbu_store_t** out);
int orbu_store_destroy(orbu_store_t* store);
int orbu_kf_set(orbu_store_t* store, const OrbuKeyFrames* kfs);
int orbu_kf_set_graph(orbu_store_t* store, const OrbuKeyFrames* kfs);
int orbu_kf_set_flags(orbu_store_t* store, const int32_t* slots, const uint8_t* flags, int n);
int orbu_kf_set_entries(orbu_store_t* store, int slot, const int32_t* idx, const int32_t* vals, int n);
int orbu_update_local_map(orbu_store_t* store, const int32_t* frame_ids, int n, int max_keyframes, OrbuResult* result);
int orbu_local_points(orbu_store_t* store, const int32_t* kf_list, int nkf, const int32_t* frame_ids, int n, OrbuResult* result);
int orbu_debug_set_generation(orbu_store_t* store, uint32_t generation);
int orbu_debug_resident_list(orbu_store_t* store, int32_t* out, int cap, int* n);
int orbw_track_local_map_resident(orbm_frameset_t* fs, int slot, orbw_pool_t* pool, orbu_store_t* store, const OrbmProjParams* pp,
                                  const OrbwView* view, float th, const float* scale_factors, const float* level_breaks, int nlevels,
                                  const uint8_t* t_occ);

#ifdef __cplusplus
}
#endif
#endif
