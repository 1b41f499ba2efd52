// iORB_SLAM::SearchLocalPointsT::RunResident (include/Tracking_hip.hpp) -- SearchLocalPoints from the list orbu_update_local_map
// left on the device -- on the mock world of localmap_dropin_gpu.cpp (its frame, MapPoints, serial reference loop and generator
// are taken as they are: that program's main is renamed away) against the same serial reference loop.  The local map is three
// keyframes that split the world's local point list in order, so UpdateLocalPoints returns that list without its bad points and
// the reference, which skips bad points itself (Tracking.cc:1230), must leave the same frame and the same counters.
// Built by tests/test_gpu_localmap_update.py; needs a GPU.
#define main localmap_dropin_main
#include "localmap_dropin_gpu.cpp"
#undef main

int main()
{
    if (orbx_device_count() == 0) { fprintf(stderr, "no HIP device: no CPU fallback\n"); return 3; }
    orbm_t* m = nullptr;
    OX(orbm_create(0, &m));
    OrbxParams prm; prm.nfeatures = 1000; prm.scaleFactor = 1.2f; prm.nlevels = NLEVELS; prm.iniThFAST = 20; prm.minThFAST = 7;
    orbx_t* ex = nullptr;
    OX(orbx_create(&prm, W, H, 1, 0, &ex));
    int total = 0;
    const int n = 479, cap = 512;
    for (int th = 1; th <= 5; th += 2) {
        World ref, dev;
        makeWorld(ref, 200u + th, n);
        makeWorld(dev, 200u + th, n);
        // (that world stamps a few points it does not hold with the frame's id; in Tracking a point carries mCurrentFrame.mnId in
        // mnLastFrameSeen only once :1216 has met it in the frame, and the resident list is defined by that)
        for (size_t i = 0; i < ref.pts.size(); i++) ref.pts[i].mnLastFrameSeen = dev.pts[i].mnLastFrameSeen = ref.F.mnId - 1;
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
        OX(orbm_frameset_create(m, 4, cap, K, D, &g, bounds, F.mvScaleFactors.data(), NLEVELS, &fs));
        OX(orbm_frameset_build(fs, 1, 1, (const OrbxKeyPoint*)dk, (const uint8_t*)dd, (const int32_t*)dn, n));
        OX(orbm_frameset_sync(fs));
        orbw_pool_t* pool = nullptr;
        OX(orbw_pool_create(m, (int)dev.pts.size(), &pool));
        std::vector<int32_t> ids(dev.pts.size());
        std::vector<OrbwPoint> recs(dev.pts.size());
        std::vector<MapPoint*> ofId(dev.pts.size());
        for (size_t i = 0; i < dev.pts.size(); i++) {
            MapPoint& p = dev.pts[i];
            ids[i] = p.poolId; ofId[(size_t)p.poolId] = &p;
            OrbwPoint& r = recs[i];
            for (int c = 0; c < 3; c++) { r.pos[c] = p.mWorldPos.at<float>(c); r.normal[c] = p.mNormalVector.at<float>(c); }
            r.min_distance = p.mfMinDistance; r.max_distance = p.mfMaxDistance;
            for (int b = 0; b < 32; b++) r.desc[b] = p.mDescriptor.ptr<unsigned char>(0)[b];
            r.flags = (uint8_t)((p.isBad() ? ORBW_FLAG_BAD : 0) | (p.Observations() > 0 ? ORBW_FLAG_OBSERVED : 0));
            r.pad[0] = r.pad[1] = r.pad[2] = 0;
        }
        OX(orbw_pool_set(pool, ids.data(), recs.data(), (int)ids.size()));
        // three keyframes hold the local list, a third each, in order
        const int nl = (int)dev.local.size(), stride = (nl + 2) / 3;
        orbu_store_t* store = nullptr;
        OX(orbu_store_create(pool, 3, stride, 0, nl, &store));
        std::vector<int32_t> entries(nl);
        for (int i = 0; i < nl; i++) entries[i] = dev.local[i]->poolId;
        const int32_t slot[3] = {0, 1, 2}, cnt[3] = {stride, stride, nl - 2 * stride}, parent[3] = {-1, -1, -1}, nch[3] = {0, 0, 0};
        const uint8_t kflags[3] = {0, 0, 0};
        int32_t neigh[30];
        for (int j = 0; j < 30; j++) neigh[j] = -1;
        OrbuKeyFrames kf;
        kf.nkf = 3; kf.slot = slot; kf.flags = kflags; kf.n = cnt; kf.entries = entries.data(); kf.neigh = neigh; kf.parent = parent; kf.nchildren = nch; kf.children = nullptr;
        OX(orbu_kf_set(store, &kf));
        std::vector<int32_t> frameIds(n, -1);
        for (int t = 0; t < n; t++) if (F.mvpMapPoints[t]) frameIds[t] = F.mvpMapPoints[t]->poolId;
        typedef iORB_SLAM::SearchLocalPointsT<Frame, MapPoint> SLP;
        SLP::Options opt; opt.th = th;
        // refused before the store's first update, with nothing touched
        bool threw = false;
        try { SLP::RunResident(fs, 1, cap, pool, store, dev.F, dev.local, opt); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { fprintf(stderr, "RunResident before the first update did not refuse\n"); return 1; }
        OrbuResult ur;
        OX(orbu_update_local_map(store, frameIds.data(), n, 80, &ur));
        if (ur.status != ORBU_OK || ur.nkf != 3) { fprintf(stderr, "update: status %d, %d keyframes\n", ur.status, ur.nkf); return 1; }
        std::vector<MapPoint*> local;
        for (int i = 0; i < ur.nL; i++) local.push_back(ofId[(size_t)ur.L[i]]);
        int wantToMatch = 0, wantMatches = 0;
        searchLocalPoints(ref.F, ref.local, th, wantToMatch, wantMatches);
        SLP::Result got;
        try { got = SLP::RunResident(fs, 1, cap, pool, store, dev.F, local, opt); } catch (const std::exception& e) { fprintf(stderr, "RunResident threw: %s\n", e.what()); return 2; }
        if (got.nToMatch != wantToMatch || got.nmatches != wantMatches) {
            fprintf(stderr, "th %d: nToMatch %d (want %d), nmatches %d (want %d)\n", th, got.nToMatch, wantToMatch, got.nmatches, wantMatches);
            return 1;
        }
        for (int t = 0; t < n; t++) {
            const long a = dev.F.mvpMapPoints[t] ? dev.F.mvpMapPoints[t]->mnId : -1, b = ref.F.mvpMapPoints[t] ? ref.F.mvpMapPoints[t]->mnId : -1;
            if (a != b) { fprintf(stderr, "th %d: feature %d holds %ld, want %ld\n", th, t, a, b); return 1; }
        }
        for (size_t i = 0; i < dev.pts.size(); i++) {
            const MapPoint &a = dev.pts[i], &b = ref.pts[i];
            if (a.mnVisible != b.mnVisible || a.mnLastFrameSeen != b.mnLastFrameSeen || a.mbTrackInView != b.mbTrackInView) {
                fprintf(stderr, "th %d: point %zu visible %d/%d lastSeen %lu/%lu inView %d/%d\n", th, i, a.mnVisible, b.mnVisible, a.mnLastFrameSeen, b.mnLastFrameSeen,
                        (int)a.mbTrackInView, (int)b.mbTrackInView);
                return 1;
            }
        }
        total += wantMatches;
        OX(orbu_store_destroy(store));
        OX(orbw_pool_destroy(pool));
        OX(orbm_frameset_destroy(fs));
        OX(orbx_device_free(ex, dk)); OX(orbx_device_free(ex, dd)); OX(orbx_device_free(ex, dn));
    }
    if (total < 300) { fprintf(stderr, "only %d matches over all scenes: the scenes do not exercise the search\n", total); return 1; }
    orbx_destroy(ex);
    orbm_destroy(m);
    printf("localmap resident dropin ok: %d matches\n", total);
    return 0;
}
