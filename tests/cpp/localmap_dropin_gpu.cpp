// iORB_SLAM::SearchLocalPointsT::Run (include/Tracking_hip.hpp) on mock frames and MapPoints (mock_tracking.hpp) against the
// serial reference loop -- Tracking::SearchLocalPoints (Tracking.cc:1206-1256) with ORBmatcher::SearchByProjection(F,
// vpMapPoints, th) (ORBmatcher.cc:45-129) -- over a copy of the same mocks: F.mvpMapPoints, every point's visible counter,
// mnLastFrameSeen and mbTrackInView, nToMatch and the match count.  Built by tests/test_gpu_localmap.py; needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "Tracking_hip.hpp"
#include "mock_tracking.hpp"
#include "dropin_test.hpp"

using tmock::Frame;
using tmock::MapPoint;
using mock::KeyPoint;
using mock::Mat;

static const int W = 640, H = 480, NLEVELS = 8, TH_HIGH = 100;

static int descriptorDistance(const Mat& a, const unsigned char* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a.ptr<unsigned char>(0)[i] ^ b[i]));
    return d;
}

static float radiusByViewingCos(const float& viewCos) { if (viewCos > 0.998) return 2.5; else return 4.0; }

// ORBmatcher.cc:45-129, monocular (mvuRight < 0 everywhere)
static int searchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th, float mfNNratio)
{
    int nmatches = 0;
    const bool bFactor = th != 1.0;
    for (size_t iMP = 0; iMP < vpMapPoints.size(); iMP++) {
        MapPoint* pMP = vpMapPoints[iMP];
        if (!pMP->mbTrackInView) continue;
        if (pMP->isBad()) continue;
        const int& nPredictedLevel = pMP->mnTrackScaleLevel;
        float r = radiusByViewingCos(pMP->mTrackViewCos);
        if (bFactor) r *= th;
        const std::vector<size_t> vIndices = F.GetFeaturesInArea(pMP->mTrackProjX, pMP->mTrackProjY, r * F.mvScaleFactors[nPredictedLevel], nPredictedLevel - 1, nPredictedLevel);
        if (vIndices.empty()) continue;
        const Mat MPdescriptor = pMP->GetDescriptor();
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        for (size_t k = 0; k < vIndices.size(); k++) {
            const size_t idx = vIndices[k];
            if (F.mvpMapPoints[idx]) if (F.mvpMapPoints[idx]->Observations() > 0) continue;
            const int dist = descriptorDistance(MPdescriptor, F.mDescriptors.ptr<unsigned char>((int)idx));
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = F.mvKeysUn[idx].octave; bestIdx = (int)idx; }
            else if (dist < bestDist2) { bestLevel2 = F.mvKeysUn[idx].octave; bestDist2 = dist; }
        }
        if (bestDist <= TH_HIGH) {
            if (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2) continue;
            F.mvpMapPoints[bestIdx] = pMP;
            nmatches++;
        }
    }
    return nmatches;
}

// Tracking.cc:1206-1256
static void searchLocalPoints(Frame& F, std::vector<MapPoint*>& local, int th, int& nToMatch, int& nmatches)
{
    for (size_t t = 0; t < F.mvpMapPoints.size(); t++) {
        MapPoint* pMP = F.mvpMapPoints[t];
        if (pMP) {
            if (pMP->isBad()) F.mvpMapPoints[t] = static_cast<MapPoint*>(NULL);
            else { pMP->IncreaseVisible(1); pMP->mnLastFrameSeen = F.mnId; pMP->mbTrackInView = false; }
        }
    }
    nToMatch = 0; nmatches = 0;
    for (size_t i = 0; i < local.size(); i++) {
        MapPoint* pMP = local[i];
        if (pMP->mnLastFrameSeen == F.mnId) continue;
        if (pMP->isBad()) continue;
        if (F.isInFrustum(pMP, 0.5)) { pMP->IncreaseVisible(1); nToMatch++; }
    }
    if (nToMatch > 0) nmatches = searchByProjection(F, local, (float)th, 0.8f);
}

struct World {
    Frame F;
    std::vector<MapPoint> pts;
    std::vector<MapPoint*> local;
};

// a frame of n features on a jittered lattice and a local map: one MapPoint per feature seen within a pixel of it plus as many
// anywhere around the frustum; some already matched in the frame, some bad, some without observations
static void makeWorld(World& w, unsigned seed, int n)
{
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    Frame& F = w.F;
    Frame::fx = 517.3f; Frame::fy = 516.5f; Frame::cx = 318.6f; Frame::cy = 255.3f;
    Frame::mnMinX = 0.f; Frame::mnMaxX = (float)W; Frame::mnMinY = 0.f; Frame::mnMaxY = (float)H;
    Frame::mfGridElementWidthInv = 64.f / W; Frame::mfGridElementHeightInv = 48.f / H;
    F.mnId = 7; F.N = n;
    F.mvScaleFactors.assign(NLEVELS, 1.f);
    for (int l = 1; l < NLEVELS; l++) F.mvScaleFactors[l] = (float)(F.mvScaleFactors[l - 1] * 1.2);
    F.mfLogScaleFactor = std::log(1.2f);
    F.mvKeysUn.resize(n); F.mDescriptors = Mat::u8(n, 32); F.mvpMapPoints.assign(n, nullptr); F.mvuRight.assign(n, -1.f);
    for (int i = 0; i < n; i++) {
        KeyPoint& k = F.mvKeysUn[i];
        k.pt.x = 8.f + U(rng) * (W - 16.f); k.pt.y = 8.f + U(rng) * (H - 16.f);
        k.octave = (int)(U(rng) * NLEVELS) % NLEVELS; k.size = 31.f * F.mvScaleFactors[k.octave]; k.angle = U(rng) * 360.f; k.response = 1.f; k.class_id = -1;
        for (int b = 0; b < 32; b++) F.mDescriptors.ptr<unsigned char>(i)[b] = (unsigned char)(rng() & 255);
    }
    F.AssignFeaturesToGrid();
    // a pose close to the identity: a small turn about y and a shift
    const float a = 0.02f, ca = std::cos(a), sa = std::sin(a);
    const float R[9] = {ca, 0.f, sa, 0.f, 1.f, 0.f, -sa, 0.f, ca}, t[3] = {0.05f, -0.02f, 0.03f};
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) F.mRcw.at<float>(r, c) = R[3 * r + c]; F.mtcw.at<float>(r) = t[r]; }
    for (int r = 0; r < 3; r++) F.mOw.at<float>(r) = -(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);   // -Rcw^T tcw
    w.pts.resize(2 * (size_t)n);
    for (int i = 0; i < 2 * n; i++) {
        MapPoint& p = w.pts[i];
        p.mnId = i; p.poolId = 2 * n - 1 - i;   // (pool ids in another order than the list)
        const bool onFeature = i < n;
        const float z = 2.f + U(rng) * 12.f;
        float u, v; int level;
        if (onFeature) { u = F.mvKeysUn[i].pt.x + (U(rng) - 0.5f) * 2.f; v = F.mvKeysUn[i].pt.y + (U(rng) - 0.5f) * 2.f; level = F.mvKeysUn[i].octave; }
        else { u = -100.f + U(rng) * (W + 200.f); v = -100.f + U(rng) * (H + 200.f); level = (int)(U(rng) * NLEVELS) % NLEVELS; }
        float Xc[3] = {(u - Frame::cx) / Frame::fx * z, (v - Frame::cy) / Frame::fy * z, (!onFeature && U(rng) < 0.1f) ? -z : z};
        float Xw[3], d[3], dist = 0.f;
        for (int r = 0; r < 3; r++) Xw[r] = R[r] * (Xc[0] - t[0]) + R[3 + r] * (Xc[1] - t[1]) + R[6 + r] * (Xc[2] - t[2]);
        for (int r = 0; r < 3; r++) { d[r] = Xw[r] - F.mOw.at<float>(r); dist += d[r] * d[r]; }
        dist = std::sqrt(dist);
        const float tilt = onFeature ? U(rng) * 0.1f : U(rng) * 1.4f;   // the normal: the view direction, tilted about a fixed axis
        for (int r = 0; r < 3; r++) { p.mWorldPos.at<float>(r) = Xw[r]; p.mNormalVector.at<float>(r) = d[r] / dist; }
        p.mNormalVector.at<float>(0) = std::cos(tilt) * d[0] / dist + std::sin(tilt) * d[2] / dist;
        p.mNormalVector.at<float>(2) = -std::sin(tilt) * d[0] / dist + std::cos(tilt) * d[2] / dist;
        p.mfMaxDistance = (onFeature ? 0.95f : 0.4f + U(rng) * 2.f) * dist * F.mvScaleFactors[level];
        p.mfMinDistance = p.mfMaxDistance / F.mvScaleFactors[NLEVELS - 1];
        for (int b = 0; b < 32; b++) {
            unsigned char byte = onFeature ? F.mDescriptors.ptr<unsigned char>(i)[b] : (unsigned char)(rng() & 255);
            if (onFeature && U(rng) < 0.08f) byte ^= (unsigned char)(1u << (rng() & 7));
            p.mDescriptor.ptr<unsigned char>(0)[b] = byte;
        }
        p.nObs = U(rng) < 0.9f ? 1 + (int)(U(rng) * 5) : 0;
        p.mbBad = U(rng) < 0.05f;
        p.mnVisible = 1 + (int)(U(rng) * 20);
        p.mnLastFrameSeen = U(rng) < 0.05f ? F.mnId : F.mnId - 1;   // (a few already stamped by this frame)
    }
    // the frame's own matches from TrackWithMotionModel: every seventh feature holds its point, a few of them bad
    for (int i = 0; i < n; i += 7) F.mvpMapPoints[i] = &w.pts[i];
    for (size_t i = 0; i < w.pts.size(); i++) w.local.push_back(&w.pts[(i * 37) % w.pts.size()]);   // (2n and 37 are coprime for the sizes used)
}

int main()
{
    if (orbx_device_count() == 0) { fprintf(stderr, "no HIP device: no CPU fallback\n"); return 3; }
    orbm_t* m = nullptr;
    OX(orbm_create(0, &m));
    OrbxParams prm; prm.nfeatures = 1000; prm.scaleFactor = 1.2f; prm.nlevels = NLEVELS; prm.iniThFAST = 20; prm.minThFAST = 7;
    orbx_t* ex = nullptr;
    OX(orbx_create(&prm, W, H, 1, 0, &ex));
    int total = 0;
    const int sizes[3] = {479, 64, 1};
    for (int rep = 0; rep < 3; rep++) {
        const int n = sizes[rep], cap = 512;
        for (int th = 1; th <= 5; th += 2) {
            World ref, dev;
            makeWorld(ref, 100u + rep, n);
            makeWorld(dev, 100u + rep, n);
            // the frame into a frame set, the MapPoints into a pool
            Frame& F = dev.F;
            std::vector<OrbxKeyPoint> keys(n);
            std::vector<uint8_t> desc((size_t)n * 32);
            for (int i = 0; i < n; i++) {
                const KeyPoint& k = F.mvKeysUn[i];
                keys[i].x = k.pt.x; keys[i].y = k.pt.y; keys[i].size = k.size; keys[i].angle = k.angle; keys[i].response = k.response; keys[i].octave = k.octave; keys[i].class_id = k.class_id;
                for (int b = 0; b < 32; b++) desc[(size_t)i * 32 + b] = F.mDescriptors.ptr<unsigned char>(i)[b];
            }
            void *dk = nullptr, *dd = nullptr, *dn = nullptr;
            OX(orbx_device_alloc(ex, keys.size() * sizeof(OrbxKeyPoint), &dk));
            OX(orbx_device_alloc(ex, desc.size(), &dd));
            OX(orbx_device_alloc(ex, 4, &dn));
            const int32_t count = n;
            OX(orbx_upload(ex, dk, keys.data(), keys.size() * sizeof(OrbxKeyPoint)));
            OX(orbx_upload(ex, dd, desc.data(), desc.size()));
            OX(orbx_upload(ex, dn, &count, 4));
            const float K[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy}, D[5] = {0, 0, 0, 0, 0}, bounds[4] = {0.f, (float)W, 0.f, (float)H};
            OrbmGrid g; g.minX = 0.f; g.minY = 0.f; g.invW = Frame::mfGridElementWidthInv; g.invH = Frame::mfGridElementHeightInv; g.cols = 64; g.rows = 48;
            orbm_frameset_t* fs = nullptr;
            OX(orbm_frameset_create(m, 2, cap, K, D, &g, bounds, F.mvScaleFactors.data(), NLEVELS, &fs));
            OX(orbm_frameset_build(fs, 1, 1, (const OrbxKeyPoint*)dk, (const uint8_t*)dd, (const int32_t*)dn, n));
            OX(orbm_frameset_sync(fs));
            orbw_pool_t* pool = nullptr;
            OX(orbw_pool_create(m, (int)dev.pts.size(), &pool));
            std::vector<int32_t> ids(dev.pts.size());
            std::vector<OrbwPoint> recs(dev.pts.size());
            for (size_t i = 0; i < dev.pts.size(); i++) {
                MapPoint& p = dev.pts[i];
                ids[i] = p.poolId;
                OrbwPoint& r = recs[i];
                for (int c = 0; c < 3; c++) { r.pos[c] = p.mWorldPos.at<float>(c); r.normal[c] = p.mNormalVector.at<float>(c); }
                r.min_distance = p.mfMinDistance; r.max_distance = p.mfMaxDistance;
                for (int b = 0; b < 32; b++) r.desc[b] = p.mDescriptor.ptr<unsigned char>(0)[b];
                r.flags = (uint8_t)((p.isBad() ? ORBW_FLAG_BAD : 0) | (p.Observations() > 0 ? ORBW_FLAG_OBSERVED : 0));
                r.pad[0] = r.pad[1] = r.pad[2] = 0;
            }
            OX(orbw_pool_set(pool, ids.data(), recs.data(), (int)ids.size()));
            int wantToMatch = 0, wantMatches = 0;
            searchLocalPoints(ref.F, ref.local, th, wantToMatch, wantMatches);
            typedef iORB_SLAM::SearchLocalPointsT<Frame, MapPoint> SLP;
            SLP::Options opt; opt.th = th;
            SLP::Result got;
            try {
                got = SLP::Run(fs, 1, cap, pool, dev.F, dev.local, [](MapPoint* p) { return p->poolId; }, opt);
            } catch (const std::exception& e) { fprintf(stderr, "Run threw: %s\n", e.what()); return 2; }
            if (got.nToMatch != wantToMatch || got.nmatches != wantMatches) {
                fprintf(stderr, "n %d th %d: nToMatch %d (want %d), nmatches %d (want %d)\n", n, th, got.nToMatch, wantToMatch, got.nmatches, wantMatches);
                return 1;
            }
            for (int t = 0; t < n; t++) {
                const long a = dev.F.mvpMapPoints[t] ? dev.F.mvpMapPoints[t]->mnId : -1, b = ref.F.mvpMapPoints[t] ? ref.F.mvpMapPoints[t]->mnId : -1;
                if (a != b) { fprintf(stderr, "n %d th %d: feature %d holds %ld, want %ld\n", n, th, t, a, b); return 1; }
            }
            for (size_t i = 0; i < dev.pts.size(); i++) {
                const MapPoint &a = dev.pts[i], &b = ref.pts[i];
                if (a.mnVisible != b.mnVisible || a.mnLastFrameSeen != b.mnLastFrameSeen || a.mbTrackInView != b.mbTrackInView) {
                    fprintf(stderr, "n %d th %d: point %zu visible %d/%d lastSeen %lu/%lu inView %d/%d\n", n, th, i, a.mnVisible, b.mnVisible, a.mnLastFrameSeen,
                            b.mnLastFrameSeen, (int)a.mbTrackInView, (int)b.mbTrackInView);
                    return 1;
                }
            }
            total += wantMatches;
            // a refusal throws with everything as it came: an id the pool never held
            if (rep == 0 && th == 1) {
                World again; makeWorld(again, 100u + rep, n);
                bool threw = false;
                try { SLP::Run(fs, 1, cap, pool, again.F, again.local, [](MapPoint* p) { return p->poolId + 100000; }, opt); } catch (const std::runtime_error&) { threw = true; }
                World fresh; makeWorld(fresh, 100u + rep, n);
                bool same = threw;
                for (int t = 0; t < n && same; t++) same = (again.F.mvpMapPoints[t] != nullptr) == (fresh.F.mvpMapPoints[t] != nullptr);
                for (size_t i = 0; i < again.pts.size() && same; i++)
                    same = again.pts[i].mnVisible == fresh.pts[i].mnVisible && again.pts[i].mnLastFrameSeen == fresh.pts[i].mnLastFrameSeen;
                if (!same) { fprintf(stderr, "a refused call changed the mocks (threw %d)\n", (int)threw); return 1; }
            }
            OX(orbw_pool_destroy(pool));
            OX(orbm_frameset_destroy(fs));
            OX(orbx_device_free(ex, dk)); OX(orbx_device_free(ex, dd)); OX(orbx_device_free(ex, dn));
        }
    }
    if (total < 300) { fprintf(stderr, "only %d matches over all scenes: the scenes do not exercise the search\n", total); return 1; }
    orbx_destroy(ex);
    orbm_destroy(m);
    printf("localmap dropin ok: %d matches\n", total);
    return 0;
}
