// PnPsolver_hip.hpp -- the reference's PnPsolver (include/PnPsolver.h, src/PnPsolver.cc of both scenarios) over the C ABI
// of liborbslamm_hip.so (orbp_*).  Header-only, C++11.
//
//   PnPsolverT<Frame, MapPoint, Mat, Random>
//       the drop-in: the reference's constructor, SetRansacParameters, find and iterate.  In the reference tree:
//           typedef iORB_SLAM::PnPsolverT<Frame, MapPoint, cv::Mat, DUtils::Random> PnPsolver;
//       The constructor does the reference's walk over vpMapPointMatches on the host (null and bad points skipped) and
//       hands the compacted lists to the device; it ends in SetRansacParameters() with the header's defaults.
//   RunAll(solvers)
//       ONE device call for all of a frame's candidates: Tracking::Relocalization builds every solver before the first
//       iterate, so call RunAll on vpPnPsolvers there (null entries, the discarded candidates, are skipped).  Without it
//       the first iterate of each solver runs its own.  After it iterate is host-only, but for the mask of a returned pose.
//   The RANSAC sets are drawn here by the reference's algorithm (PnPsolver.cc:191-201: Random::RandomInt over the
//   process's rand(), the overwrite at the drawn VALUE included), mRansacMaxIts + 4 sets of a solver (what iterate(5) can
//   reach: its loop is an OR) BEFORE the device call.  The reference draws a set only when it reaches that iteration, so
//   after an early return its rand() stream is less advanced than here: each solver's results are those of the reference
//   given the same sets, the process-wide rand() stream afterwards is not.  A call that would pass
//   the sets drawn so far -- iterate(5) on a candidate still live past mRansacMaxIts because the caller rejected its Refine
//   returns, find() after an iterate, an nIterations above 5 -- draws the missing sets at that moment and the device
//   continues the solver's table (orbp_run on a solver that has iterated), as the reference's loop simply goes on.
//   It is a template so that it compiles (and is tested, tests/cpp/pnp_dropin_gpu.cpp) without OpenCV: Mat needs a
//   (rows, cols, type) constructor, a default one (empty) and at<float>(r, c).
//   Every call runs on the calling thread's matcher handle (orbm_thread_handle), as the other drop-ins do.
#pragma once

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

template <class Frame, class MapPoint, class Mat, class Random>
class PnPsolverT {
public:
    static const int kExtraSets = 4;

    // PnPsolver(const Frame& F, const vector<MapPoint*>& vpMapPointMatches)
    PnPsolverT(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches, int device = 0)
    {
        mNAll = (int)vpMapPointMatches.size();
        std::vector<int32_t> idx;
        std::vector<float> p2d, s2, p3d;
        for (int i = 0; i < mNAll; i++) {
            MapPoint* pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            p2d.push_back(F.mvKeysUn[i].pt.x);
            p2d.push_back(F.mvKeysUn[i].pt.y);
            s2.push_back(F.mvLevelSigma2[F.mvKeysUn[i].octave]);
            const auto Pos = pMP->GetWorldPos();
            for (int r = 0; r < 3; r++) p3d.push_back(Pos.template at<float>(r, 0));
            idx.push_back(i);
        }
        N = (int)idx.size();
        const float K[4] = {F.fx, F.fy, F.cx, F.cy};
        orbm_t* h = nullptr;
        check(orbm_thread_handle(device, &h));
        check(orbp_create(h, mNAll, idx.data(), N, p2d.data(), s2.data(), p3d.data(), K, &s_));
        readBack();
    }
    ~PnPsolverT() { orbp_destroy(s_); }
    PnPsolverT(const PnPsolverT&) = delete;
    PnPsolverT& operator=(const PnPsolverT&) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991)
    {
        check(orbp_set_ransac(s_, probability, minInliers, maxIterations, minSet, epsilon, th2));
        readBack();
        ran_ = false;
    }

    // cv::Mat find(vector<bool>& vbInliers, int& nInliers)
    Mat find(std::vector<bool>& vbInliers, int& nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }

    // cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)
    Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        if (!ran_ && N >= mRansacMinInliers) RunAll(std::vector<PnPsolverT*>(1, this));
        // the loop is an OR: this call can evaluate hypotheses up to max(mnIterations + nIterations, mRansacMaxIts).  A
        // candidate whose Refine returns are rejected by the caller stays live past mRansacMaxIts (a Refine return never
        // sets bNoMore), and find() after an iterate asks for mRansacMaxIts more: draw what is missing and let the device
        // continue the table, the state kept
        if (N >= mRansacMinInliers) {
            const long want = std::max((long)res_.iterations + (nIterations > 0 ? nIterations : 0), (long)mRansacMaxIts);
            const long have = (long)(sets_.size() / 4);
            if (want > have) extend((int)(want - have));
        }
        mask_.assign((size_t)mNAll + 1, 0);
        check(orbp_iterate(s_, nIterations, &res_, mask_.data()));
        bNoMore = res_.no_more != 0;
        nInliers = res_.n_inliers;
        vbInliers.clear();   // (the reference fills it only when it returns a pose)
        if (!res_.returned) return Mat();
        vbInliers = detail::mask_bools(mask_, mNAll);
        return detail::mat32f<Mat>(res_.Tcw, 4, 4);
    }

    // every hypothesis of every solver in one device call; the sets are drawn solver by solver, in list order
    static void RunAll(const std::vector<PnPsolverT*>& solvers)
    {
        std::vector<PnPsolverT*> live;
        std::vector<orbp_t*> hs;
        std::vector<const int32_t*> ps;
        std::vector<int32_t> ns;
        for (size_t i = 0; i < solvers.size(); i++) {
            PnPsolverT* s = solvers[i];
            if (!s) continue;
            const bool draws = s->N >= s->mRansacMinInliers;
            if (draws) s->drawSets();
            live.push_back(s);
            hs.push_back(s->s_);
            ps.push_back(draws ? s->sets_.data() : nullptr);
            ns.push_back(draws ? s->mRansacMaxIts + kExtraSets : 0);
        }
        if (hs.empty()) return;
        check(orbp_run(hs.data(), (int)hs.size(), ps.data(), ns.data()));
        for (size_t i = 0; i < live.size(); i++) live[i]->ran_ = true;
    }

    // the last iterate's result (the returning hypothesis, mnIterations, mnBestInliers) and the sets drawn
    const OrbpResult& lastResult() const { return res_; }
    const std::vector<int32_t>& sets() const { return sets_; }
    int correspondences() const { return N; }
    int maxIterations() const { return mRansacMaxIts; }
    int minInliers() const { return mRansacMinInliers; }

private:
    void readBack()
    {
        check(orbp_max_iterations(s_, &mRansacMaxIts));
        check(orbp_min_inliers(s_, &mRansacMinInliers));
    }
    // iterate's draw (PnPsolver.cc:191-201) for mRansacMaxIts + kExtraSets iterations
    void drawSets() { sets_.clear(); drawMore(mRansacMaxIts + kExtraSets); }
    // `count` more hypotheses behind the table: their sets drawn now, evaluated by a run that continues the table
    void extend(int count)
    {
        // (a solver that has not iterated yet has no table to continue: it is run again on all its sets)
        const size_t from = (res_.iterations || res_.best_inliers) ? sets_.size() : 0;
        drawMore(count);
        orbp_t* h = s_;
        const int32_t* p = sets_.data() + from;
        const int32_t n = (int32_t)((sets_.size() - from) / 4);
        check(orbp_run(&h, 1, &p, &n));
    }
    void drawMore(int count) { detail::draw_sets<Random>(N, 4, count, sets_); }
    static void check(int rc) { detail::check(rc, "PnPsolver(HIP): "); }

    int N = 0, mNAll = 0, mRansacMinInliers = 8, mRansacMaxIts = 300;
    bool ran_ = false;
    orbp_t* s_ = nullptr;
    OrbpResult res_{};
    std::vector<int32_t> sets_;
    std::vector<uint8_t> mask_;
};

}  // namespace iORB_SLAM
