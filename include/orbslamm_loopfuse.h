/* orbslamm_loopfuse.h -- the SearchAndFuse block of liborbslamm_hip.so's C ABI.  Included by
 * orbslamm_hip.h, whose types it uses (through orbslamm_fuse.h: OrblFuseTarget, OrblFusePoint, the ORBL_FUSE_ST_* codes and
 * the break table of orbl_level_breaks); including any of the three headers gives all. */
#ifndef ORBSLAMM_LOOPFUSE_H
#define ORBSLAMM_LOOPFUSE_H
#include "orbslamm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------------------
 * LoopClosing::SearchAndFuse (src/LoopClosing.cc:601-627) and MultiMapper::SearchAndFuse (src/MultiMapper.cc:668-694),
 * monocular: the searches of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:979-1102) of EVERY
 * point against EVERY target keyframe in one call.  The shape is dense, T x P, so there is no job list; and
 * the result is sparse, so what comes back is an ordered list of hits and not one record per pair.  The search of one
 * point in one target (:1010-1081) depends on no other pair.  What is serial (isBad, spAlreadyFound, GetMapPoint,
 * vpReplacePoint, AddObservation, Replace) is the caller's, at replay (include/LoopClosing_hip.hpp).  Pure functions of
 * their arguments: the same call twice gives identical bytes.
 *
 * targets: OrblFuseTarget as orbl_fuse_batch takes it.  The caller decomposes Scw (ORBmatcher.cc:987-992) into Rcw, tcw and
 *   Ow; K, the image bounds and the grid are the keyframe's.  A keyframe may appear as several targets (with other poses or
 *   the same); host arrays given twice (the same keys_un, desc, n and grid) go up once, a frame listed twice is referenced
 *   twice and uploaded never.
 * points: OrblFusePoint, the pool every target searches (64 bytes a point, uploaded once per call).
 * Per pair (target k, point i): the five projection gates of §8l in orbx_cvmath.hpp's forms (depth, image bounds, distance
 *   range, viewing angle, the predicted level from the break table), radius = th * scale_factors[level], the window in
 *   GetFeaturesInArea's order with the level window [level - 1, level] and the strict `<` (the first candidate in walk order
 *   wins a tie).  There is NO chi-square test in this Fuse.  invz is `1.0/z` rounded to float at :1021; a correctly rounded
 *   float division gives the same bits (binary64 carries more than 2 * 24 + 2 bits; tests/test_loopfuse_cpu.py sweeps it).
 * hits: a pair with best_idx >= 0 && best_dist <= max_dist (the drop-in passes TH_LOW).  OrbcHit records come target-major,
 *   points ascending inside a target; hit_start[k] .. hit_start[k + 1] is target k's stretch (hit_start may be NULL).
 * status: when given, one ORBL_FUSE_ST_* byte per pair at status[k * n_points + i]; FOUND means a best exists, whatever its
 *   distance.  For tests and diagnosis: production passes NULL and nothing of size T x P crosses the link.
 * capacity: more hits than `capacity` return ORBX_E_CAPACITY with *n_hits the needed count; hits, hit_start and status
 *   are then left unwritten.  hits may be NULL when capacity is 0.
 * Limits and refusals (refused, never truncated; the argument checks come before the handle's and need no GPU):
 *   ORBX_E_UNSUPPORTED above ORBC_MAX_TARGETS targets or ORBC_MAX_PAIRS pairs (n_targets * n_points).  The ceilings: the
 *   kernels keep one 4-byte word per pair in HBM between the search and the compaction (256 MiB at 2^26 pairs; a merge of
 *   1000 keyframes and 8000 points is 2^23), every pair index stays inside int32 with room to spare, and one workgroup
 *   scans the at most 2^26 / 128 + 8192 tile counts in well under a millisecond.
 *   ORBX_E_INVALID for null arguments, negative counts, more than 65535 features in a target, a bad grid, a break table
 *   that does not ascend strictly, nlevels outside [1, 16], max_dist outside [0, 256], a negative capacity.
 *   Zero targets or zero points: ORBX_OK, *n_hits = 0 (and hit_start all zero).  A target without features gives
 *   NO_CANDIDATE for every pair that passes the gates.  No CPU fallback. */
#define ORBC_MAX_TARGETS 8192
#define ORBC_MAX_PAIRS (1 << 26)
typedef struct {
    int32_t target, point, best_idx, best_dist;
} OrbcHit;
int orbc_search_and_fuse(orbm_t* h, const OrblFuseTarget* targets, const OrbxKeyPoint* const* keys_un, const uint8_t* const* desc,
                         const int32_t* n, int n_targets, const OrblFusePoint* points, int n_points, float th, int max_dist,
                         const float* scale_factors, int nlevels, const float* level_breaks, OrbcHit* hits, int capacity, int* n_hits,
                         int32_t* hit_start /* n_targets + 1, may be NULL */, uint8_t* status /* n_targets * n_points, may be NULL */);
int orbc_search_and_fuse_frames(orbm_t* h, const OrblFuseTarget* targets, orbm_frame_t* const* frames, int n_targets,
                                const OrblFusePoint* points, int n_points, float th, int max_dist, const float* scale_factors,
                                int nlevels, const float* level_breaks, OrbcHit* hits, int capacity, int* n_hits,
                                int32_t* hit_start /* n_targets + 1, may be NULL */, uint8_t* status /* n_targets * n_points, may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
