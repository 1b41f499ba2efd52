/* orbslamm_reloc.h -- the block of liborbslamm_hip.so's C ABI that closes Tracking::Relocalization behind PnPsolver::iterate on
 * the device.  Included by orbslamm_hip.h, whose types it uses (orbm_t, orbm_frameset_t, orbw_pool_t,
 * orbu_store_t, OrboFrame, OrboResult, the ORBX_* codes); including either gives both. */
#ifndef ORBSLAMM_RELOC_H
#define ORBSLAMM_RELOC_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * Tracking::Relocalization, the body behind PnPsolver::iterate (Tracking.cc:1486-1547, monocular), for any number of independent
 * jobs in ONE call.  A job is (lost frame, candidate keyframe, the pose and inliers a PnP iterate returned).  Everything read is
 * resident: positions, distance bounds, descriptors and the bad bit in the map-point pool, the keyframe's match row in the
 * keyframe store, the frame's mvKeysUn, grid and descriptors and the keyframe's angles in frame-set slots.
 *
 * A job: fs, slot = the resident mCurrentFrame; kf_slot = the candidate as a slot of fs (only its angles are read, for the
 *   rotation histogram); kf = the candidate's slot in the store (its entries row is GetMapPointMatches()); n = mCurrentFrame.N;
 *   ids[n] for :1492-1501: the pool id of vvpMapPointMatches[i][t] where vbInliers[t], else -1; frame = PnP's Tcw (:1486) and K.
 * Call-wide: check_ori (matcher2's, :1459), inv_level_sigma2, scale_factors, level_breaks (orbl_level_breaks) and nlevels.  The
 *   image bounds are the frame set's.
 *
 * The rules, in the order they run:
 * 1. Solve 1 (:1503).  Edges are the features with ids[t] >= 0 in ASCENDING t (Optimizer.cc:302-341); Xw is the pool record's
 *    pos, the observation the resident mvKeysUn[t]; the solve is orbo_pose_optimize_frames' own (section 8o).  Below 3 edges
 *    nGood = 0 and the pose stays as it came.  nGood < 10: exit REJECTED (:1505; the frame keeps the ids as they came, the pose
 *    the solve left).  Otherwise outliers lose their point (:1508-1510).  nGood >= 50: exit FIRST (:1513).
 * 2. sFound (:1488, :1497) is the set of the job's ids[t] >= 0 AS THEY CAME IN, solve 1's outliers included.  Membership is by
 *    pool id and exact, and one job's membership never depends on another job's (two candidates commonly share points).
 * 3. Wide search (:1515: SearchByProjection(mCurrentFrame, pKF, sFound, 10, 100), ORBmatcher.cc:1474-1601), per entry q of the
 *    row: e = entries[kf][q]; e == -1, or q at or above the store's stride, or an id outside the pool: NO_POINT.  Otherwise id =
 *    e & ~ORBU_ENTRY_NO_VOTE (a point in the match slot takes part).  Pool flag bit 0: BAD (:1496).  A member of sFound: FOUND
 *    (:1496).  Rcw, tcw from the job's CURRENT Tcw, the pose solve 1 left (:1478-1479).  Ow = -Rcw.t()*tcw (:1480): per
 *    component the double sum over k of Rcw(k,i)*tcw[k], times -1.0, narrowed.  x3Dc = Rcw*x3Dw + tcw (:1500) in gemm's small
 *    form: the three float products summed left to right, then (float)((double)t*1.0 + (double)tcw[i]*1.0).  invzc =
 *    (float)(1.0 / (double)z) (:1504); there is NO depth gate, the reference has none: a point behind the camera that lands
 *    inside the image goes on.  u = fx*xc*invzc + cx, v alike, float, left to right (:1506-1507).  Not (u >= min && u <= max),
 *    or the same for v: OUT_OF_IMAGE (:1509-1512; a NaN u or v too: the pool's defined choice).  dist3D = (float)norm(x3Dw - Ow),
 *    the squares summed in double (:1515-1516).  dist3D < 0.8f*min || dist3D > 1.2f*max: DISTANCE (:1522).  The level
 *    (:1525 PredictScale): the number of breaks below RAW max / dist3D, less one, as the pool's projections count it; outside
 *    [0, nlevels): LEVEL_RANGE.  radius = th * scale_factors[level] (:1528), the level window [level - 1, level + 1] (:1530):
 *    IN_VIEW.  The query descriptor is the POOL record's (:1535), the angle the keyframe slot's key q (:1564).
 *    The search is orbm_search_by_projection's mode 5 (sections 8b, 8q): a feature that holds a point NOW is occupied (:1543),
 *    strict < in GetFeaturesInArea's order (:1550), best <= ORBdist (:1557), a matched feature is occupied for the entries
 *    behind it, the rotation histogram and its three maxima under check_ori (:1562-1597).  nadditional = its count behind the
 *    pruning (:1600).  A matched feature takes the row's pool id (:1559).  nadditional + nGood < 50: exit WIDE_SHORT (:1517);
 *    the frame keeps the added points.
 * 4. Solve 2 (:1519) over every feature that holds a point, from the pose solve 1 left.  Outliers are NOT discarded.
 *    nGood >= 50 or nGood <= 30: exit SECOND (:1523).
 * 5. Narrow search (:1525-1529): sFound rebuilt from every feature that holds a point, solve 2's outliers included; th = 3,
 *    ORBdist = 64, the pose solve 2 left.  nGood + nadditional < 50: exit NARROW_SHORT (:1532).
 * 6. Solve 3 (:1534-1538) with the discard: exit THIRD.
 * 7. Out, per job: exit; n_good[3] and n_additional[2], 0 where not reached; opt[3], zero where not reached; Tcw as
 *    mCurrentFrame.mTcw is left; ids_out[n] as mvpMapPoints is left at that exit; outlier_out[n]: 0 or 1 as the LAST solve of
 *    the job that had feature t as an edge left mvbOutlier[t], and ORBQ_RELOC_KEEP where no solve of the job had an edge at t
 *    (the reference leaves that flag as the previous candidate left it; such a flag never reaches a job's ids or counts: at
 *    :1508 and :1536 a feature without an edge holds no point).  The verdict nGood >= 50 (:1546) is the caller's:
 *    orbq_reloc_n_good gives the nGood the verdict reads.  status_out[j], where given: 2 * stride bytes, the wide projection's
 *    status per row entry and then the narrow one's; ORBQ_RELOC_ST_NOT_RUN where the job did not reach that search.
 * A feature at or above n takes no part (it is occupied for both searches); n above the slot's device count is fine as long as
 *   no feature there holds a point.
 *
 * The call: synchronous, ONE synchronise, a fixed number of launches whatever the number of jobs or their exits; one packed
 *   upload (job records | ids) and one copy down.  Jobs may name different frame sets of h, the same keyframe or frame several
 *   times; a job's bytes do not depend on its neighbours, and the same call twice gives the same bytes.  The scratch is the
 *   handle's own: no result set of the frame sets' rings is taken or disturbed.  The pool's mutex (the store shares it) is held
 *   from the checks to the synchronise, and the call leaves the reader event orbw_pool_set* and orbu_* wait for.  It runs on
 *   the handle's stream, behind the slots' builds.
 * Candidate arena: a search whose candidates pass the job's share of the arena reports its need and the job stops; the host
 *   grows the arena to the largest need reported and runs the WHOLE call again (it has written nothing but its own scratch, so
 *   the second run is exact) -- at most twice, the wide search's need being settled by the first re-run and the narrow one's by
 *   the second.  Partial results are never returned.  orbq_debug_reloc_arena sets the share's starting size in entries, for
 *   tests (0: the default, 8 entries a row entry).
 * Refusals (never truncations; the argument checks come first and need no GPU):
 *   n_jobs == 0: ORBX_OK at once, nothing read or written.
 *   ORBX_E_UNSUPPORTED above ORBO_MAX_FRAMES jobs, n above ORBO_MAX_EDGES, more than ORBO_MAX_CALL_EDGES features a call, or
 *   jobs whose frame sets' caps add up to more than ORBO_MAX_CALL_EDGES.
 *   ORBX_E_INVALID for null arguments, n < 0 or above the set's cap, a negative slot, check_ori outside {0, 1}, nlevels outside
 *   [1, 16], a break table that does not ascend strictly, a slot outside the set, a frame set of another handle, a store of
 *   another pool, kf outside the store or not set, an id outside the pool or never set, a store whose stride is above the
 *   frame set's cap; and, found by a kernel and reported behind it with the outputs unwritten: an edge's octave outside
 *   [0, nlevels), a feature with a point at or above the slot's device count, a row entry with a point at or above the keyframe
 *   slot's device count.
 *   ORBX_E_CAPACITY when the arena still overflows in the third run.
 *   No CPU fallback. */
typedef struct {
    orbm_frameset_t* fs;
    int32_t slot;       /* mCurrentFrame */
    int32_t kf_slot;    /* the candidate keyframe as a slot of fs: its angles */
    int32_t kf;         /* its slot in the store: entries[kf][q] */
    int32_t n;          /* mCurrentFrame.N */
    const int32_t* ids; /* [n] */
    OrboFrame frame;    /* PnP's Tcw and K */
} OrbqRelocJob;
#define ORBQ_RELOC_REJECTED 0      /* :1505 nGood < 10 */
#define ORBQ_RELOC_FIRST 1         /* :1513 nGood >= 50 behind solve 1 */
#define ORBQ_RELOC_WIDE_SHORT 2    /* :1517 */
#define ORBQ_RELOC_SECOND 3        /* :1523 */
#define ORBQ_RELOC_NARROW_SHORT 4  /* :1532 */
#define ORBQ_RELOC_THIRD 5         /* :1534-1538 */
#define ORBQ_RELOC_KEEP 0xff
#define ORBQ_RELOC_ST_NOT_RUN 0
#define ORBQ_RELOC_ST_NO_POINT 1
#define ORBQ_RELOC_ST_BAD 2
#define ORBQ_RELOC_ST_FOUND 3
#define ORBQ_RELOC_ST_OUT_OF_IMAGE 4
#define ORBQ_RELOC_ST_DISTANCE 5
#define ORBQ_RELOC_ST_LEVEL_RANGE 6
#define ORBQ_RELOC_ST_IN_VIEW 7
typedef struct {
    OrboResult opt[3];
    float Tcw[16];
    int32_t exit;
    int32_t n_good[3];
    int32_t n_additional[2];
} OrbqRelocResult;
int orbq_relocalize(orbm_t* h, orbw_pool_t* pool, orbu_store_t* store, const OrbqRelocJob* jobs, int n_jobs, int check_ori,
                    const float* inv_level_sigma2, const float* scale_factors, const float* level_breaks, int nlevels,
                    OrbqRelocResult* out, int32_t* const* ids_out /* [n_jobs][n] */, uint8_t* const* outlier_out /* [n_jobs][n] */,
                    uint8_t* const* status_out /* may be null, or hold nulls: [n_jobs][2 * stride] */);
/* the nGood that :1546 reads at the job's exit */
static inline int orbq_reloc_n_good(const OrbqRelocResult* r)
{
    return r->exit == ORBQ_RELOC_THIRD ? r->n_good[2] : r->exit == ORBQ_RELOC_SECOND || r->exit == ORBQ_RELOC_NARROW_SHORT ? r->n_good[1] : r->n_good[0];
}
/* for the tests of the overflow path: entries_per_job >= 0 sets the starting size of a job's share of the candidate arena (0: the
 * default; what the arena has grown to is dropped), -1 leaves it; last_runs, where given, gets how many times the last
 * orbq_relocalize on h ran its chain (1: no overflow; at most 3) */
int orbq_debug_reloc_arena(orbm_t* h, int entries_per_job, int* last_runs);

#ifdef __cplusplus
}
#endif
#endif
