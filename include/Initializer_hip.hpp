// Initializer_hip.hpp -- the reference's Initializer (include/Initializer.h, src/Initializer.cc of both scenarios) over
// the C ABI of liborbslamm_hip.so (orbi_*).  Header-only, C++11.
//
//   InitializerT<Frame, Mat, Point3f, Random, kHF>
//       the drop-in: the reference's constructor and Initialize signature.  In the reference tree:
//           typedef iORB_SLAM::InitializerT<Frame, cv::Mat, cv::Point3f, DUtils::Random> Initializer;          // SingleRobot
//           typedef iORB_SLAM::InitializerT<Frame, cv::Mat, cv::Point3f, DUtils::Random, false> Initializer;   // MultipleRobots
//       kHF selects the scenario: true = FindHomography and FindFundamental with the RH > 0.45 choice (SingleRobotScenario),
//       false = FindFundamental and ReconstructF only (MultipleRobotsScenario).
//       The RANSAC sets are drawn here exactly as the reference draws them (Initializer.cc:67-97): Random::SeedRandOnce(0),
//       then Random::RandomInt over the process's rand(), the same calls in the same order; the device then runs the rest.
//       It is a template so that it compiles (and is tested, tests/cpp/init_dropin_gpu.cpp) without OpenCV: Frame needs
//       mvKeysUn (cv::KeyPoint-layout records) and mK (at<float>(r, c)); Mat a (rows, cols, type) constructor, a default
//       one (empty) and at<float>(r, c); Point3f a (x, y, z) constructor.
//   Every call runs on the calling thread's matcher handle (orbm_thread_handle), as the other drop-ins do.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "orbslamm_dropin.hpp"
#include "orbslamm_hip.h"

namespace iORB_SLAM {

template <class Frame, class Mat, class Point3f, class Random, bool kHF = true>
class InitializerT {
public:
    // Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200)
    InitializerT(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200, int device = 0)
        : mSigma(sigma), mMaxIterations(iterations), n1_((int)ReferenceFrame.mvKeysUn.size())
    {
        const float K[4] = {ReferenceFrame.mK.template at<float>(0, 0), ReferenceFrame.mK.template at<float>(1, 1),
                            ReferenceFrame.mK.template at<float>(0, 2), ReferenceFrame.mK.template at<float>(1, 2)};
        orbm_t* h = nullptr;
        check(orbm_thread_handle(device, &h));
        check(orbi_create(h, reinterpret_cast<const OrbxKeyPoint*>(ReferenceFrame.mvKeysUn.data()), n1_, K, sigma, iterations,
                          kHF ? ORBI_MODEL_HF : ORBI_MODEL_F, &ini_));
    }
    ~InitializerT() { orbi_destroy(ini_); }
    InitializerT(const InitializerT&) = delete;
    InitializerT& operator=(const InitializerT&) = delete;

    // bool Initialize(const Frame& CurrentFrame, const vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21,
    //                 vector<cv::Point3f>& vP3D, vector<bool>& vbTriangulated)
    bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, Mat& R21, Mat& t21, std::vector<Point3f>& vP3D,
                    std::vector<bool>& vbTriangulated)
    {
        if ((int)vMatches12.size() != n1_) throw std::runtime_error("Initializer(HIP): vMatches12 must have one entry per reference key");
        int N = 0;
        for (size_t i = 0; i < vMatches12.size(); i++) if (vMatches12[i] >= 0) N++;
        // (fewer than 8 matches: the reference draws from an empty vector; refused below, before any draw)
        if (N >= 8) drawSets(N);
        else sets_.assign((size_t)mMaxIterations * 8, 0);
        m12_.assign(vMatches12.begin(), vMatches12.end());
        p3d_.resize((size_t)n1_ * 3 + 3);
        tri_.resize((size_t)n1_ + 1);
        check(orbi_initialize(ini_, reinterpret_cast<const OrbxKeyPoint*>(CurrentFrame.mvKeysUn.data()), (int)CurrentFrame.mvKeysUn.size(),
                              m12_.data(), sets_.data(), &res_, p3d_.data(), tri_.data()));
        if (res_.rt_state == 1) { R21 = Mat(); t21 = Mat(); }
        if (res_.rt_state == 2) {
            R21 = detail::mat32f<Mat>(res_.R21, 3, 3);
            t21 = detail::mat32f<Mat>(res_.t21, 3, 1);
        }
        if (res_.ok) {
            vP3D.clear();
            vP3D.reserve((size_t)n1_);
            vbTriangulated.assign((size_t)n1_, false);
            for (int i = 0; i < n1_; i++) {
                vP3D.push_back(Point3f(p3d_[3 * i], p3d_[3 * i + 1], p3d_[3 * i + 2]));
                vbTriangulated[i] = tri_[i] != 0;
            }
        }
        return res_.ok != 0;
    }

    // the last call's diagnostics (scores, winning hypotheses, every candidate's nGood and parallax)
    const OrbiResult& lastResult() const { return res_; }

    float mSigma;
    int mMaxIterations;

private:
    void drawSets(int N)
    {
        std::vector<size_t> vAllIndices, vAvailableIndices;
        vAllIndices.reserve(N);
        for (int i = 0; i < N; i++) vAllIndices.push_back(i);
        sets_.assign((size_t)mMaxIterations * 8, 0);
        Random::SeedRandOnce(0);
        for (int it = 0; it < mMaxIterations; it++) {
            vAvailableIndices = vAllIndices;
            for (size_t j = 0; j < 8; j++) {
                const int randi = Random::RandomInt(0, vAvailableIndices.size() - 1);
                const int idx = vAvailableIndices[randi];
                sets_[(size_t)it * 8 + j] = idx;
                vAvailableIndices[randi] = vAvailableIndices.back();
                vAvailableIndices.pop_back();
            }
        }
    }
    static void check(int rc) { detail::check(rc, "Initializer(HIP): "); }

    int n1_;
    orbi_t* ini_ = nullptr;
    OrbiResult res_{};
    std::vector<int32_t> m12_, sets_;
    std::vector<float> p3d_;
    std::vector<uint8_t> tri_;
};

}  // namespace iORB_SLAM
