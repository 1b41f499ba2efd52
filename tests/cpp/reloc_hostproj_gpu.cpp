// iORB_SLAM::ORBmatcherT::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (include/ORBmatcher_hip.hpp: the host
// gates of :549-571 in front of orbm_search_by_projection_frame, mode 5) on mocks filled from a scene that tests/test_gpu_reloc.py
// writes: which row entries it pushed as queries, how many matches it made and what the frame's points are behind it go back to the
// test, which holds orbq_relocalize's wide search to them.
//     reloc_hostproj_gpu <in> <out>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <vector>

#include "ORBmatcher_hip.hpp"
#include "mock_slam.hpp"

using namespace mock;
typedef iORB_SLAM::ORBmatcherT<Frame, KeyFrame, MapPoint> ORBmatcher;

template <class T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); } }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[6];   // n, nk, npool, nlevels, th, ORBdist
    rd(f, hd, 6);
    const int n = hd[0], nk = hd[1], npool = hd[2], nlevels = hd[3];
    float cam[10], Tcw[16], logsf;   // fx fy cx cy, minX maxX minY maxY, grid invW invH
    rd(f, cam, 10); rd(f, Tcw, 16); rd(f, &logsf, 1);
    std::vector<float> sf((size_t)nlevels);
    rd(f, sf.data(), sf.size());
    std::vector<KeyPoint> keys((size_t)n);
    rd(f, keys.data(), keys.size());
    std::vector<uint8_t> desc((size_t)n * 32), found((size_t)npool), pflags((size_t)npool), pdesc((size_t)npool * 32);
    std::vector<int32_t> cur((size_t)n), entries((size_t)nk);
    std::vector<float> kang((size_t)nk), pos((size_t)npool * 3), minD((size_t)npool), maxD((size_t)npool);
    rd(f, desc.data(), desc.size()); rd(f, cur.data(), cur.size()); rd(f, found.data(), found.size()); rd(f, entries.data(), entries.size());
    rd(f, kang.data(), kang.size()); rd(f, pos.data(), pos.size()); rd(f, minD.data(), minD.size()); rd(f, maxD.data(), maxD.size());
    rd(f, pflags.data(), pflags.size()); rd(f, pdesc.data(), pdesc.size());
    std::fclose(f);

    std::vector<std::unique_ptr<MapPoint> > mps((size_t)npool);
    for (int i = 0; i < npool; i++) {
        mps[(size_t)i].reset(new MapPoint());
        MapPoint& p = *mps[(size_t)i];
        p.id = i;
        for (int k = 0; k < 3; k++) p.mWorldPos.at<float>(k, 0) = pos[3 * (size_t)i + k];
        for (int k = 0; k < 32; k++) p.mDescriptor.at<uint8_t>(0, k) = pdesc[32 * (size_t)i + k];
        p.mfMinDistance = minD[(size_t)i]; p.mfMaxDistance = maxD[(size_t)i];
        p.mbBad = (pflags[(size_t)i] & 1) != 0;
    }
    Frame::fx = cam[0]; Frame::fy = cam[1]; Frame::cx = cam[2]; Frame::cy = cam[3];
    Frame::mnMinX = cam[4]; Frame::mnMaxX = cam[5]; Frame::mnMinY = cam[6]; Frame::mnMaxY = cam[7];
    Frame::mfGridElementWidthInv = cam[8]; Frame::mfGridElementHeightInv = cam[9];
    Frame F;
    F.N = n; F.mvKeys = keys; F.mvKeysUn = keys;
    F.mvuRight.assign((size_t)n, -1.f);
    F.mDescriptors = Mat::u8(n, 32);
    for (int t = 0; t < n; t++) for (int k = 0; k < 32; k++) F.mDescriptors.at<uint8_t>(t, k) = desc[32 * (size_t)t + k];
    F.mvpMapPoints.assign((size_t)n, nullptr);
    F.mvbOutlier.assign((size_t)n, false);
    for (int t = 0; t < n; t++) if (cur[(size_t)t] >= 0) F.mvpMapPoints[(size_t)t] = mps[(size_t)cur[(size_t)t]].get();
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) F.mTcw.at<float>(r, c) = Tcw[4 * r + c];
    F.mvScaleFactors = sf; F.mfLogScaleFactor = logsf;
    KeyFrame kf;
    kf.N = nk; kf.mvKeysUn.resize((size_t)nk); kf.mvpMapPoints.assign((size_t)nk, nullptr);
    for (int q = 0; q < nk; q++) {
        kf.mvKeysUn[(size_t)q].angle = kang[(size_t)q];
        if (entries[(size_t)q] >= 0) kf.mvpMapPoints[(size_t)q] = mps[(size_t)(entries[(size_t)q] & ~(1 << 30))].get();
    }
    std::set<MapPoint*> sFound;
    for (int i = 0; i < npool; i++) if (found[(size_t)i]) sFound.insert(mps[(size_t)i].get());

    ORBmatcher m(0.9f, true);
    const int32_t nmatches = m.SearchByProjection(F, &kf, sFound, (float)hd[4], hd[5]);
    const ORBmatcher::FlatCall& c = m.last();
    std::vector<uint8_t> pushed((size_t)nk, 0);
    for (int q = 0; q < c.nq; q++) pushed[(size_t)c.qidx[(size_t)q]] = 1;
    std::vector<int32_t> ids((size_t)n, -1);
    for (int t = 0; t < n; t++) if (F.mvpMapPoints[(size_t)t]) ids[(size_t)t] = F.mvpMapPoints[(size_t)t]->id;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int32_t nq = c.nq;
    std::fwrite(&nmatches, 4, 1, o); std::fwrite(&nq, 4, 1, o);
    std::fwrite(ids.data(), 4, ids.size(), o); std::fwrite(pushed.data(), 1, pushed.size(), o);
    std::fclose(o);
    std::printf("reloc hostproj ok: %d queries, %d matches\n", (int)nq, (int)nmatches);
    return 0;
}
