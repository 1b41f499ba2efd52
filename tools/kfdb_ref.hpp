// kfdb_ref.hpp -- a literal C++ restatement of KeyFrameDatabase (src/KeyFrameDatabase.cc) and DBoW2's L1Scoring::score,
// on any KeyFrame / Frame type with the reference's members (mnId, mBowVec, the six query fields,
// GetBestCovisibilityKeyFrames(10)).  The checker of tests/cpp/kfdb_dropin_gpu.cpp and the CPU side of
// tools/kfdb_bench.py; single-threaded (no mutex).
#ifndef KFDB_REF_HPP
#define KFDB_REF_HPP

#include <cmath>
#include <list>
#include <set>
#include <utility>
#include <vector>

namespace kfdb_ref {

template <class BowVector>
double l1_score(const BowVector& v1, const BowVector& v2)
{
    typename BowVector::const_iterator a = v1.begin(), b = v2.begin();
    double s = 0;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) {
            const double vi = a->second, wi = b->second;
            s += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            ++a; ++b;
        } else if (a->first < b->first) {
            a = v1.lower_bound(b->first);
        } else {
            b = v2.lower_bound(a->first);
        }
    }
    s = -s / 2.0;
    return s;
}

template <class KeyFrame, class Frame>
class Database {
public:
    explicit Database(size_t nWords) : mInv(nWords), mN(0) {}

    void add(KeyFrame* k)
    {
        mN++;
        for (typename BowOf::const_iterator it = k->mBowVec.begin(); it != k->mBowVec.end(); ++it) mInv[it->first].push_back(k);
    }
    void erase(KeyFrame* k)
    {
        if (mN > 0) mN--;
        for (typename BowOf::const_iterator it = k->mBowVec.begin(); it != k->mBowVec.end(); ++it) {
            std::list<KeyFrame*>& l = mInv[it->first];
            for (typename std::list<KeyFrame*>::iterator li = l.begin(); li != l.end(); ++li)
                if (*li == k) { l.erase(li); break; }
        }
    }
    void clear()
    {
        const size_t n = mInv.size();
        mInv.clear();
        mInv.resize(n);
    }
    int size() const { return mN; }
    bool empty() const { return mN == 0; }

    std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* q, float minScore)
    {
        const std::set<KeyFrame*> conn = q->GetConnectedKeyFrames();
        std::list<KeyFrame*> shared;
        for (typename BowOf::const_iterator it = q->mBowVec.begin(); it != q->mBowVec.end(); ++it) {
            std::list<KeyFrame*>& l = mInv[it->first];
            for (typename std::list<KeyFrame*>::iterator li = l.begin(); li != l.end(); ++li) {
                KeyFrame* k = *li;
                if (k->mnLoopQuery != q->mnId) {
                    k->mnLoopWords = 0;
                    if (!conn.count(k)) { k->mnLoopQuery = q->mnId; shared.push_back(k); }
                }
                k->mnLoopWords++;
            }
        }
        if (shared.empty()) return std::vector<KeyFrame*>();
        int maxW = 0;
        for (typename std::list<KeyFrame*>::iterator li = shared.begin(); li != shared.end(); ++li) if ((*li)->mnLoopWords > maxW) maxW = (*li)->mnLoopWords;
        const int minW = maxW * 0.8f;
        std::list<std::pair<float, KeyFrame*> > scored;
        for (typename std::list<KeyFrame*>::iterator li = shared.begin(); li != shared.end(); ++li) {
            KeyFrame* k = *li;
            if (k->mnLoopWords > minW) {
                const float si = (float)l1_score(q->mBowVec, k->mBowVec);
                k->mLoopScore = si;
                if (si >= minScore) scored.push_back(std::make_pair(si, k));
            }
        }
        if (scored.empty()) return std::vector<KeyFrame*>();
        std::list<std::pair<float, KeyFrame*> > acc;
        float bestAcc = minScore;
        for (typename std::list<std::pair<float, KeyFrame*> >::iterator it = scored.begin(); it != scored.end(); ++it) {
            const std::vector<KeyFrame*> nb = it->second->GetBestCovisibilityKeyFrames(10);
            float best = it->first, a = it->first;
            KeyFrame* pb = it->second;
            for (size_t i = 0; i < nb.size(); i++) {
                KeyFrame* k2 = nb[i];
                if (k2->mnLoopQuery == q->mnId && k2->mnLoopWords > minW) {
                    a += k2->mLoopScore;
                    if (k2->mLoopScore > best) { pb = k2; best = k2->mLoopScore; }
                }
            }
            acc.push_back(std::make_pair(a, pb));
            if (a > bestAcc) bestAcc = a;
        }
        return retain(acc, bestAcc);
    }

    std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F)
    {
        std::list<KeyFrame*> shared;
        for (typename BowOf::const_iterator it = F->mBowVec.begin(); it != F->mBowVec.end(); ++it) {
            std::list<KeyFrame*>& l = mInv[it->first];
            for (typename std::list<KeyFrame*>::iterator li = l.begin(); li != l.end(); ++li) {
                KeyFrame* k = *li;
                if (k->mnRelocQuery != F->mnId) { k->mnRelocWords = 0; k->mnRelocQuery = F->mnId; shared.push_back(k); }
                k->mnRelocWords++;
            }
        }
        if (shared.empty()) return std::vector<KeyFrame*>();
        int maxW = 0;
        for (typename std::list<KeyFrame*>::iterator li = shared.begin(); li != shared.end(); ++li) if ((*li)->mnRelocWords > maxW) maxW = (*li)->mnRelocWords;
        const int minW = maxW * 0.8f;
        std::list<std::pair<float, KeyFrame*> > scored;
        for (typename std::list<KeyFrame*>::iterator li = shared.begin(); li != shared.end(); ++li) {
            KeyFrame* k = *li;
            if (k->mnRelocWords > minW) {
                const float si = (float)l1_score(F->mBowVec, k->mBowVec);
                k->mRelocScore = si;
                scored.push_back(std::make_pair(si, k));
            }
        }
        if (scored.empty()) return std::vector<KeyFrame*>();
        std::list<std::pair<float, KeyFrame*> > acc;
        float bestAcc = 0;
        for (typename std::list<std::pair<float, KeyFrame*> >::iterator it = scored.begin(); it != scored.end(); ++it) {
            const std::vector<KeyFrame*> nb = it->second->GetBestCovisibilityKeyFrames(10);
            float best = it->first, a = best;
            KeyFrame* pb = it->second;
            for (size_t i = 0; i < nb.size(); i++) {
                KeyFrame* k2 = nb[i];
                if (k2->mnRelocQuery != F->mnId) continue;
                a += k2->mRelocScore;
                if (k2->mRelocScore > best) { pb = k2; best = k2->mRelocScore; }
            }
            acc.push_back(std::make_pair(a, pb));
            if (a > bestAcc) bestAcc = a;
        }
        return retain(acc, bestAcc);
    }

private:
    typedef typename KeyFrame::BowVector BowOf;
    std::vector<std::list<KeyFrame*> > mInv;
    int mN;

    static std::vector<KeyFrame*> retain(const std::list<std::pair<float, KeyFrame*> >& acc, float bestAcc)
    {
        const float thr = 0.75f * bestAcc;
        std::set<KeyFrame*> seen;
        std::vector<KeyFrame*> out;
        for (typename std::list<std::pair<float, KeyFrame*> >::const_iterator it = acc.begin(); it != acc.end(); ++it)
            if (it->first > thr && !seen.count(it->second)) { out.push_back(it->second); seen.insert(it->second); }
        return out;
    }
};

}  // namespace kfdb_ref

#endif
