// Sim3Solver_hip.hpp -- the reference's Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc of both scenarios) over the
// C ABI of liborbslamm_hip.so (orbs_*).  Header-only, C++11.
//
//   Sim3SolverT<KeyFrame, MapPoint, Mat, Random>
//       the drop-in: the reference's constructor, SetRansacParameters, find, iterate and GetEstimated*.  In the reference tree:
//           typedef iORB_SLAM::Sim3SolverT<KeyFrame, MapPoint, cv::Mat, DUtils::Random> Sim3Solver;
//       The constructor does the reference's walk over vpMatched12 on the host (null / bad points, GetIndexInKeyFrame) and
//       hands the compacted lists to the device.  The intrinsics are read from the keyframe's fx, fy, cx, cy (what mK is
//       built from).
//   RunAll(solvers)
//       ONE device call for all of a query's candidates: MultiMapper::Run and LoopClosing::ComputeSim3 build every solver
//       before the first iterate, so call RunAll on the list there.  Without it the first iterate of each solver runs its own.
//   The RANSAC sets are drawn here by the reference's algorithm (Sim3Solver.cc:163-177: Random::RandomInt over the
//   process's rand(), the overwrite at the drawn VALUE included), all mRansacMaxIts sets of a solver BEFORE the device
//   call.  The reference draws a set only when it reaches that iteration, so after an early return its rand() stream is
//   less advanced than here: each solver's results are those of the reference given the same sets, the process-wide
//   rand() stream afterwards is not.
//   It is a template so that it compiles (and is tested, tests/cpp/sim3_dropin_gpu.cpp) without OpenCV: Mat needs a
//   (rows, cols, type) constructor, a default one (empty) and at<float>(r, c).
//   Every call runs on the calling thread's matcher handle (orbm_thread_handle), as the other drop-ins do.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

template <class KeyFrame, class MapPoint, class Mat, class Random>
class Sim3SolverT {
public:
    // Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12, const bool bFixScale = true)
    Sim3SolverT(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true, int device = 0)
    {
        std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        std::vector<int32_t> idx1;
        std::vector<float> X1w, X2w, s1, s2;
        for (int i1 = 0; i1 < mN1; i1++) {
            if (!vpMatched12[i1]) continue;
            MapPoint* pMP1 = vpKeyFrameMP1[i1];
            MapPoint* pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
            const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            s1.push_back(pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave]);
            s2.push_back(pKF2->mvLevelSigma2[pKF2->mvKeysUn[indexKF2].octave]);
            idx1.push_back(i1);
            push3(X1w, pMP1->GetWorldPos());
            push3(X2w, pMP2->GetWorldPos());
        }
        N = (int)idx1.size();
        float R1[9], t1[3], R2[9], t2[3];
        pose(pKF1, R1, t1);
        pose(pKF2, R2, t2);
        const float K1[4] = {pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy}, K2[4] = {pKF2->fx, pKF2->fy, pKF2->cx, pKF2->cy};
        orbm_t* h = nullptr;
        check(orbm_thread_handle(device, &h));
        check(orbs_create(h, mN1, idx1.data(), N, X1w.data(), X2w.data(), R1, t1, R2, t2, K1, K2, s1.data(), s2.data(), bFixScale ? 1 : 0, &s_));
        check(orbs_max_iterations(s_, &mRansacMaxIts));
    }
    ~Sim3SolverT() { orbs_destroy(s_); }
    Sim3SolverT(const Sim3SolverT&) = delete;
    Sim3SolverT& operator=(const Sim3SolverT&) = delete;

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        check(orbs_set_ransac(s_, probability, minInliers, maxIterations));
        check(orbs_max_iterations(s_, &mRansacMaxIts));
        mRansacMinInliers = minInliers;
        ran_ = false;
    }

    // cv::Mat find(vector<bool>& vbInliers12, int& nInliers)
    Mat find(std::vector<bool>& vbInliers12, int& nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    // cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)
    Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        if (!ran_ && N >= mRansacMinInliers) RunAll(std::vector<Sim3SolverT*>(1, this));
        mask_.assign((size_t)mN1 + 1, 0);
        check(orbs_iterate(s_, nIterations, &res_, mask_.data()));
        bNoMore = res_.no_more != 0;
        nInliers = res_.n_inliers;
        vbInliers = detail::mask_bools(mask_, mN1);
        return res_.returned ? detail::mat32f<Mat>(res_.T12, 4, 4) : Mat();
    }

    Mat GetEstimatedRotation() { return res_.has_best ? detail::mat32f<Mat>(res_.best_R, 3, 3) : Mat(); }
    Mat GetEstimatedTranslation() { return res_.has_best ? detail::mat32f<Mat>(res_.best_t, 3, 1) : Mat(); }
    float GetEstimatedScale() { return res_.best_s; }

    // every hypothesis of every solver in one device call; the sets are drawn solver by solver, in list order
    static void RunAll(const std::vector<Sim3SolverT*>& solvers)
    {
        std::vector<orbs_t*> hs;
        std::vector<const int32_t*> ps;
        for (size_t i = 0; i < solvers.size(); i++) {
            Sim3SolverT* s = solvers[i];
            if (s->N >= s->mRansacMinInliers) s->drawSets();
            hs.push_back(s->s_);
            ps.push_back(s->N >= s->mRansacMinInliers ? s->sets_.data() : nullptr);
        }
        if (hs.empty()) return;
        check(orbs_run(hs.data(), (int)hs.size(), ps.data()));
        for (size_t i = 0; i < solvers.size(); i++) solvers[i]->ran_ = true;
    }

    // the last iterate's result (the returning hypothesis, mnIterations, mnBestInliers) and the sets drawn
    const OrbsResult& lastResult() const { return res_; }
    const std::vector<int32_t>& sets() const { return sets_; }
    int correspondences() const { return N; }
    int maxIterations() const { return mRansacMaxIts; }

private:
    template <class M> static void push3(std::vector<float>& v, const M& m) { for (int r = 0; r < 3; r++) v.push_back(m.template at<float>(r, 0)); }
    static void pose(KeyFrame* pKF, float R[9], float t[3])
    {
        const auto Rm = pKF->GetRotation();
        const auto tm = pKF->GetTranslation();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) R[3 * r + c] = Rm.template at<float>(r, c);
            t[r] = tm.template at<float>(r, 0);
        }
    }
    // iterate's draw (Sim3Solver.cc:163-177) for all mRansacMaxIts iterations
    void drawSets() { sets_.clear(); detail::draw_sets<Random>(N, 3, mRansacMaxIts, sets_); }
    static void check(int rc) { detail::check(rc, "Sim3Solver(HIP): "); }

    int N = 0, mN1 = 0, mRansacMinInliers = 6, mRansacMaxIts = 300;
    bool ran_ = false;
    orbs_t* s_ = nullptr;
    OrbsResult res_{};
    std::vector<int32_t> sets_;
    std::vector<uint8_t> mask_;
};

}  // namespace iORB_SLAM
