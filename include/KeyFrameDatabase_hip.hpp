// KeyFrameDatabase_hip.hpp -- drop-in for KeyFrameDatabase (include/KeyFrameDatabase.h of the reference) and
// ORBVocabulary::score on the device keyframe database (orbk_* / orbv_score in orbslamm_hip.h).
//
// KeyFrameDatabaseT<KeyFrame, Frame> has the reference's members (add, erase, clear, size, empty, DetectLoopCandidates,
// DetectRelocalizationCandidates) and reads the reference's members of KeyFrame / Frame: mnId, mBowVec (a std::map-like
// BowVector: word id -> value), GetConnectedKeyFrames() and GetBestCovisibilityKeyFrames(10).  Keyframes are slots of a
// KeyFramePoolT, which may be shared by several databases (MultiMapper: one database per map).  A keyframe's six query
// fields live on the device, in its slot; the adapter mirrors none of them.
//
// A keyframe gets a slot the first time the adapter sees it through add() or a loop query (as the query or one of its
// connected keyframes).  A neighbour that GetBestCovisibilityKeyFrames(10) names and that has no slot is left out of
// the accumulation: such a keyframe was never in a database or a query, so its mnRelocQuery / mnLoopQuery are still 0
// and its scores 0.0f -- it could only count for a query id of 0, where it adds +0.0f to a positive score and never
// beats it: the same result.
//
// Threads: Tracking (relocalisation), LoopClosing (add, loop queries) and KeyFrame::SetBadFlag (erase) call one database
// at once, as in the reference.  Every member of every database over a pool holds the pool's adapter mutex for its whole
// duration, C calls included, so the adapter's maps are never read and written at once.  Lock order: the adapter mutex,
// then the C pool's lock; the neighbour callback runs on the querying thread under both and takes neither.  It calls
// GetBestCovisibilityKeyFrames (the KeyFrame's own mutex); the reference never calls the database while holding a
// KeyFrame's mutex, so no cycle forms.
//
// Errors of the C ABI are thrown as std::runtime_error.
#ifndef KEYFRAMEDATABASE_HIP_HPP
#define KEYFRAMEDATABASE_HIP_HPP

#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbslamm_hip.h"

namespace orbslamm_hip {

inline void kfdb_check(int rc, const char* what)
{
    if (rc != ORBX_OK) throw std::runtime_error(std::string(what) + ": " + orbx_last_error());
}

template <class BowVector>
inline void kfdb_flatten(const BowVector& v, std::vector<uint32_t>& ids, std::vector<double>& vals)
{
    ids.clear(); vals.clear();
    for (typename BowVector::const_iterator it = v.begin(); it != v.end(); ++it) { ids.push_back((uint32_t)it->first); vals.push_back((double)it->second); }
}

// double ORBVocabulary::score(const BowVector&, const BowVector&) (L1_NORM)
template <class BowVector>
class ORBVocabularyScoreT {
public:
    explicit ORBVocabularyScoreT(orbv_t* voc) : mpVoc(voc) {}
    double score(const BowVector& v1, const BowVector& v2) const
    {
        std::vector<uint32_t> a, b; std::vector<double> av, bv;
        kfdb_flatten(v1, a, av); kfdb_flatten(v2, b, bv);
        double s = 0;
        kfdb_check(orbv_score(mpVoc, a.data(), av.data(), (int)a.size(), b.data(), bv.data(), (int)b.size(), &s), "ORBVocabulary::score");
        return s;
    }
private:
    orbv_t* mpVoc;
};

// KeyFrame* <-> pool slot; one pool serves every database of a System (or of a MultiMapper)
template <class KeyFrame>
class KeyFramePoolT {
public:
    explicit KeyFramePoolT(orbv_t* voc) { kfdb_check(orbk_pool_create(voc, 1024, &mpPool), "orbk_pool_create"); }
    ~KeyFramePoolT() { orbk_pool_destroy(mpPool); }
    orbk_pool_t* handle() const { return mpPool; }
    // held by every KeyFrameDatabaseT member over this pool; the members below assume it is held
    std::mutex& mutex() { return mMu; }

    // the keyframe's slot, made (with its mBowVec) on first sight; an empty BowVector is uploaded again once it is computed
    int slot(KeyFrame* pKF)
    {
        typename std::map<KeyFrame*, Entry>::iterator it = mSlots.find(pKF);
        if (it != mSlots.end() && (it->second.words > 0 || pKF->mBowVec.empty() || it->second.inDb > 0)) return it->second.slot;
        const int s = it != mSlots.end() ? it->second.slot : (int)mKFs.size();
        std::vector<uint32_t> ids; std::vector<double> vals;
        kfdb_flatten(pKF->mBowVec, ids, vals);
        kfdb_check(orbk_pool_set_bow(mpPool, s, ids.data(), vals.data(), (int)ids.size()), "orbk_pool_set_bow");
        if (it == mSlots.end()) { mSlots[pKF] = Entry{s, (int)ids.size(), 0}; mKFs.push_back(pKF); }
        else it->second.words = (int)ids.size();
        return s;
    }
    int find(KeyFrame* pKF) const
    {
        typename std::map<KeyFrame*, Entry>::const_iterator it = mSlots.find(pKF);
        return it == mSlots.end() ? -1 : it->second.slot;
    }
    KeyFrame* keyframe(int slot) const { return mKFs[(size_t)slot]; }
    void held(KeyFrame* pKF, int d) { mSlots[pKF].inDb += d; }

private:
    struct Entry { int slot, words, inDb; };
    orbk_pool_t* mpPool = nullptr;
    std::mutex mMu;
    std::map<KeyFrame*, Entry> mSlots;
    std::vector<KeyFrame*> mKFs;
    KeyFramePoolT(const KeyFramePoolT&);
    KeyFramePoolT& operator=(const KeyFramePoolT&);
};

template <class KeyFrame, class Frame>
class KeyFrameDatabaseT {
public:
    typedef KeyFramePoolT<KeyFrame> Pool;

    // KeyFrameDatabase(const ORBVocabulary&): a pool of its own
    explicit KeyFrameDatabaseT(orbv_t* voc) : mpOwned(new Pool(voc)), mpPool(mpOwned) { init(); }
    // one database of several over a shared pool
    explicit KeyFrameDatabaseT(Pool* pool) : mpOwned(nullptr), mpPool(pool) { init(); }
    ~KeyFrameDatabaseT()
    {
        {
            std::lock_guard<std::mutex> lk(mpPool->mutex());
            orbk_db_destroy(mpDb);
        }
        delete mpOwned;
    }

    void add(KeyFrame* pKF)
    {
        std::lock_guard<std::mutex> lk(mpPool->mutex());
        const int s = mpPool->slot(pKF);
        kfdb_check(orbk_db_add(mpDb, s), "KeyFrameDatabase::add");
        mpPool->held(pKF, 1);
        mCopies[pKF]++;
    }
    void erase(KeyFrame* pKF)
    {
        std::lock_guard<std::mutex> lk(mpPool->mutex());
        const int s = mpPool->slot(pKF);
        kfdb_check(orbk_db_erase(mpDb, s), "KeyFrameDatabase::erase");
        typename std::map<KeyFrame*, int>::iterator it = mCopies.find(pKF);
        if (it != mCopies.end() && it->second > 0) { it->second--; mpPool->held(pKF, -1); }
    }
    void clear()
    {
        std::lock_guard<std::mutex> lk(mpPool->mutex());
        kfdb_check(orbk_db_clear(mpDb), "KeyFrameDatabase::clear");
        for (typename std::map<KeyFrame*, int>::iterator it = mCopies.begin(); it != mCopies.end(); ++it) mpPool->held(it->first, -it->second);
        mCopies.clear();
    }
    int size()
    {
        std::lock_guard<std::mutex> lk(mpPool->mutex());
        int n = 0;
        kfdb_check(orbk_db_size(mpDb, &n), "KeyFrameDatabase::size");
        return n;
    }
    bool empty()
    {
        std::lock_guard<std::mutex> lk(mpPool->mutex());
        int e = 0;
        kfdb_check(orbk_db_empty(mpDb, &e), "KeyFrameDatabase::empty");
        return e != 0;
    }

    std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore)
    {
        std::lock_guard<std::mutex> lk(mpPool->mutex());
        const int s = mpPool->slot(pKF);
        std::set<KeyFrame*> conn = pKF->GetConnectedKeyFrames();
        std::vector<int32_t> c;
        for (typename std::set<KeyFrame*>::iterator it = conn.begin(); it != conn.end(); ++it) c.push_back(mpPool->slot(*it));
        std::vector<int32_t> out(mCap());
        int n = 0;
        kfdb_check(orbk_detect_loop_candidates(mpDb, s, (uint64_t)pKF->mnId, c.data(), (int)c.size(), minScore, &neighbours, this,
                                               out.data(), (int)out.size(), &n), "KeyFrameDatabase::DetectLoopCandidates");
        return toKFs(out, n);
    }

    std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F)
    {
        std::lock_guard<std::mutex> lk(mpPool->mutex());
        std::vector<uint32_t> ids; std::vector<double> vals;
        kfdb_flatten(F->mBowVec, ids, vals);
        std::vector<int32_t> out(mCap());
        int n = 0;
        kfdb_check(orbk_detect_relocalization_candidates(mpDb, (uint64_t)F->mnId, ids.data(), vals.data(), (int)ids.size(), &neighbours, this,
                                                         out.data(), (int)out.size(), &n), "KeyFrameDatabase::DetectRelocalizationCandidates");
        return toKFs(out, n);
    }

    orbk_db_t* handle() const { return mpDb; }

private:
    Pool* mpOwned;
    Pool* mpPool;
    orbk_db_t* mpDb = nullptr;
    std::map<KeyFrame*, int> mCopies;

    void init()
    {
        std::lock_guard<std::mutex> lk(mpPool->mutex());
        kfdb_check(orbk_db_create(mpPool->handle(), &mpDb), "orbk_db_create");
    }
    size_t mCap() const
    {
        int n = 0;
        kfdb_check(orbk_pool_size(mpPool->handle(), &n), "orbk_pool_size");
        return (size_t)(n > 0 ? n : 1);
    }
    std::vector<KeyFrame*> toKFs(const std::vector<int32_t>& out, int n) const
    {
        std::vector<KeyFrame*> v;
        v.reserve((size_t)n);
        for (int i = 0; i < n; i++) v.push_back(mpPool->keyframe(out[(size_t)i]));
        return v;
    }
    // pKFi->GetBestCovisibilityKeyFrames(10) while the query runs, on the querying thread (which holds the adapter mutex
    // and the C pool's lock: no lock and no pool call in here)
    static int neighbours(void* user, int32_t slot, int32_t* out)
    {
        KeyFrameDatabaseT* self = static_cast<KeyFrameDatabaseT*>(user);
        std::vector<KeyFrame*> nb = self->mpPool->keyframe(slot)->GetBestCovisibilityKeyFrames(10);
        int k = 0;
        for (size_t i = 0; i < nb.size() && k < 10; i++) {
            const int s = self->mpPool->find(nb[i]);
            if (s >= 0) out[k++] = s;
        }
        return k;
    }
    KeyFrameDatabaseT(const KeyFrameDatabaseT&);
    KeyFrameDatabaseT& operator=(const KeyFrameDatabaseT&);
};

}  // namespace orbslamm_hip

#endif
