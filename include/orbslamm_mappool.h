/* orbslamm_mappool.h -- the map-point pool block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (orbm_t, orbm_frameset_t, OrbmProjParams, the ORBX_* codes); including either header
 * gives both. */
#ifndef ORBSLAMM_MAPPOOL_H
#define ORBSLAMM_MAPPOOL_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * Tracking::SearchLocalPoints (src/Tracking.cc:1206-1256) and the projection loop of SearchByProjection(CurrentFrame,
 * LastFrame) (src/ORBmatcher.cc:1353-1392), monocular, from MapPoints that LIVE in HBM.  A MapPoint's position, normal,
 * distance bounds and descriptor change when LocalMapping touches the point, not per frame: a pool holds them under ids the
 * caller chooses, and the two tracking searches run from a pose and a list of pool ids.  Per frame 4 bytes per point and
 * one view record go up instead of the 48 bytes per point of orbm_track_local_points; Frame::isInFrustum's loop
 * (src/Frame.cc:269-325) runs on the device (k_view_project), the search kernels are those of orbm_track_local_points.
 *
 * The pool.  orbw_pool_create: `capacity` slots, zero-initialised, none set.  Above ORBW_POOL_MAX_CAPACITY:
 *   ORBX_E_UNSUPPORTED.  OrbwPoint is OrblFusePoint's fields (GetWorldPos, GetNormal, the RAW mfMinDistance /
 *   mfMaxDistance, GetDescriptor) plus one flags byte: bit 0 isBad(), bit 1 Observations() > 0.
 *   orbw_pool_set writes n records under ids[i]; orbw_pool_set_flags changes the flags byte of ids that are already set.
 *   Both return with the update COMPLETE on the device.  They first wait for the projection kernel of every search issued
 *   against the pool (the event each search leaves), so a search in flight never reads a half-written record; a search
 *   issued later reads the new records.  The pool has a mutex: LocalMapping's thread may update while Tracking's thread
 *   searches.  An id repeated within one call takes the LAST record.  The host keeps one "set" bit per slot: every id is
 *   validated on the host before any launch.  Ids outside [0, capacity), or (searches, set_flags) never set:
 *   ORBX_E_INVALID.  Argument checks come before the handle's and need no GPU; n == 0 returns ORBX_OK at once.
 *
 * The view record, taken from the caller as OrblFuseTarget takes its fields: mRcw, mtcw, mOw of the frame, K = (fx, fy, cx,
 *   cy), mnMinX, mnMaxX, mnMinY, mnMaxY and (local-map gate set) the viewingCosLimit of Tracking.cc:1238 (0.5).
 *
 * LOCAL-MAP gate set: Frame::isInFrustum + the head of SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:45-69), per id:
 *   flags bit 0 -> BAD (Tracking.cc:1235, ORBmatcher.cc:57).  Pc = mRcw*P + mtcw (gemm's small branch with a C); PcZ < 0.0f
 *   -> DEPTH; invz = 1.0f / PcZ in float; u = fx*PcX*invz + cx, v alike, float, left to right; u < min || u > max (inclusive
 *   on both sides) -> OUT_OF_IMAGE; PO = P - mOw; dist = (float)cv::norm(PO); dist < 0.8f*min || dist > 1.2f*max -> DISTANCE;
 *   viewCos = (float)(PO.dot(Pn) / dist), the dot in double; viewCos < limit -> VIEW_ANGLE; PredictScale: ratio = RAW max /
 *   dist, level from the caller's orbl_level_breaks table exactly as orbl_fuse_batch counts it.  Then r =
 *   RadiusByViewingCos(viewCos) (2.5f when (double)viewCos > 0.998, else 4.0f), times th only when th != 1.0, times
 *   mvScaleFactors[level]; q_lvl = level - 1, level; qvalid = IN_VIEW; qobs = flags bit 1 (q_obs_pos of
 *   orbm_track_local_points).
 * FRAME/FRAME gate set: ORBmatcher.cc:1353-1392, monocular (no bForward / bBackward).  ids[i] belongs to LastFrame's feature
 *   i: the pool id of its MapPoint, or -1 for "no MapPoint or mvbOutlier[i]" -> NO_POINT (so is a feature index at or above
 *   the resident LastFrame's count).  x3Dc = Rcw*x3Dw + tcw; invzc = (float)(1.0 / z): the division is DOUBLE here; invzc < 0
 *   -> DEPTH; u, v and the bounds as above; the octave is the resident LastFrame key's; radius = th * mvScaleFactors[octave];
 *   level window [octave - 1, octave + 1].  The bad flag is NOT consulted (the reference does not); qobs = flags bit 1.
 * DEFINED CHOICES, where the reference is undefined:
 *   - a predicted level outside [0, nlevels) ends at LEVEL_RANGE and is not searched (the reference indexes
 *     mvScaleFactors out of bounds); a NaN ratio falls here by the break-table rule (above no break);
 *   - a u or v that is NaN ends at OUT_OF_IMAGE (PcZ == 0 with PcX == 0: in the reference both comparisons are false and
 *     GetFeaturesInArea converts a NaN to int).
 * What a query that is not IN_VIEW reports: u, v are 0 until the depth gate is passed; viewcos is 0 until it is formed; r
 *   is 0 unless IN_VIEW; the level is -1 until PredictScale has run, and for LEVEL_RANGE -1 (below level 0, or NaN) or
 *   nlevels; lvl = (level - 1, level).  Frame/frame: lvl = (octave - 1, octave + 1) for every id >= 0, (0, 0) for NO_POINT;
 *   viewcos stays 0.
 *
 * orbw_view_project / orbw_view_project_frame: the projection kernel alone, synchronous (the unit the parity tests hold to
 *   tools/frustum_ref.hpp).  out_uvr[3 nq], out_lvl[2 nq], out_viewcos[nq], out_status[nq]; any may be NULL.  The frame
 *   form reads the octaves of slot `last_slot` of `fs`; nq <= the set's cap.
 * orbw_track_local_map: orbm_track_local_points with the query block made on the device: asynchronous, ONE launch
 *   (k_view_project, which also brings the call's staging block up) + the two of the search, no host synchronisation, no
 *   allocation after the first call of a size.  The table comes back through orbm_track_results as ONE pair (assign[t] = the
 *   position in `ids` of the MapPoint feature t took, or -1); the status bytes lie in the set's pinned block behind the same
 *   flag: orbw_track_status(fs, back, &status, &nq) after orbm_track_results(fs, back, ..).  The caller lists the local
 *   points that pass Tracking.cc:1233 (mnLastFrameSeen != mnId); the device applies the bad flag.  pp->mode 3.  t_occ[cap] as
 *   orbm_track_local_points (NULL: none).
 * orbw_track_frame_pose: the same for orbm_track_frame_projected (pp->mode 4 or 5, rotation check from the resident
 *   LastFrame's angles); last_ids[nq], nq <= cap.
 * An arena overflow is replayed by orbm_track_results from the query block the projection kernel left in the set's own
 *   device block -- the pool is not read again, so an update in between does not change the answer -- under the refusals
 *   of every query search (ORBX_E_CAPACITY when a slot it read was rebuilt or its staging reallocated).
 * Ceilings are the query searches' own (nq <= slots * cap, <= 65536); nq == 0 is legal.  The pool and the frame set (or
 *   handle) must be on one device.  nlevels in [1, 16]; level_breaks[nlevels + 1] ascends strictly.  No CPU fallback. */
#define ORBW_POOL_MAX_CAPACITY (1 << 22)
#define ORBW_FLAG_BAD 1       /* isBad() */
#define ORBW_FLAG_OBSERVED 2  /* Observations() > 0 */
#define ORBW_ST_BAD 0           /* flags bit 0 (local-map gate set only) */
#define ORBW_ST_DEPTH 1         /* PcZ < 0.0f (Frame.cc:283) | invzc < 0 (ORBmatcher.cc:1369) */
#define ORBW_ST_OUT_OF_IMAGE 2  /* Frame.cc:291-294 | ORBmatcher.cc:1375-1378, and a NaN u or v */
#define ORBW_ST_DISTANCE 3      /* Frame.cc:302 */
#define ORBW_ST_VIEW_ANGLE 4    /* Frame.cc:310 */
#define ORBW_ST_LEVEL_RANGE 5   /* the predicted level outside [0, nlevels) */
#define ORBW_ST_IN_VIEW 6
#define ORBW_ST_NO_POINT 7      /* frame/frame gate set: id -1 */
typedef struct {
    float pos[3], normal[3];
    float min_distance, max_distance;
    uint8_t desc[32];
    uint8_t flags;
    uint8_t pad[3];
} OrbwPoint;
typedef struct {
    float Rcw[9], tcw[3], Ow[3], K[4];
    float min_x, max_x, min_y, max_y;
    float viewing_cos_limit;
} OrbwView;
typedef struct orbw_pool orbw_pool_t;
int orbw_pool_create(orbm_t* h, int capacity, orbw_pool_t** out);
int orbw_pool_destroy(orbw_pool_t* pool);
int orbw_pool_set(orbw_pool_t* pool, const int32_t* ids, const OrbwPoint* pts, int n);
int orbw_pool_set_flags(orbw_pool_t* pool, const int32_t* ids, const uint8_t* flags, int n);
int orbw_view_project(orbm_t* h, orbw_pool_t* pool, const OrbwView* view, const int32_t* ids, int nq, float th,
                      const float* scale_factors, const float* level_breaks, int nlevels, float* out_uvr, int8_t* out_lvl,
                      float* out_viewcos, uint8_t* out_status);
int orbw_view_project_frame(orbm_frameset_t* fs, int last_slot, orbw_pool_t* pool, const OrbwView* view, const int32_t* last_ids,
                            int nq, float th, const float* scale_factors, float* out_uvr, int8_t* out_lvl, uint8_t* out_status);
int orbw_track_local_map(orbm_frameset_t* fs, int slot, orbw_pool_t* pool, const OrbmProjParams* pp, const OrbwView* view,
                         const int32_t* ids, int nq, float th, const float* scale_factors, const float* level_breaks, int nlevels,
                         const uint8_t* t_occ);
int orbw_track_frame_pose(orbm_frameset_t* fs, int cur_slot, int last_slot, orbw_pool_t* pool, const OrbmProjParams* pp,
                          const OrbwView* view, const int32_t* last_ids, int nq, float th, const float* scale_factors,
                          const uint8_t* t_occ);
/* the status bytes of the search orbm_track_results(fs, back, ..) has just returned: a view into the set's pinned block,
 * valid as long as that table.  ORBX_E_INVALID when that search was not issued from a pool. */
int orbw_track_status(orbm_frameset_t* fs, int back, const uint8_t** status, int* nq);

#ifdef __cplusplus
}
#endif
#endif
