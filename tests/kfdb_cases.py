"""A literal Python restatement of KeyFrameDatabase (src/KeyFrameDatabase.cc) and DBoW2's L1Scoring::score -- the
checker of the device keyframe database -- and a random scene generator.

Keyframes are objects with the reference's six query fields; the inverted file is a list per word; scores are doubles
summed in word order and narrowed to float32 where the reference narrows; every float comparison is float32."""
import numpy as np

from vocab_cases import make_vocab

F32 = np.float32


class KeyFrame:
    def __init__(self, slot, ids=(), vals=()):
        self.slot = slot
        self.mnId = slot
        self.ids = [int(i) for i in ids]
        self.vals = [float(v) for v in vals]
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = 0, 0, F32(0.0)
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, F32(0.0)   # (the scores: the defined initial value)

    @property
    def bow(self):
        return self.ids, self.vals


def l1_score(v1, v2):
    """L1Scoring::score(v1, v2): the common words ascending, score += fabs(vi - wi) - fabs(vi) - fabs(wi), -score/2.0"""
    (a_ids, a_vals), (b_ids, b_vals) = v1, v2
    i = j = 0
    score = 0.0
    while i < len(a_ids) and j < len(b_ids):
        if a_ids[i] == b_ids[j]:
            vi, wi = float(a_vals[i]), float(b_vals[j])
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif a_ids[i] < b_ids[j]:
            i += 1
        else:
            j += 1
    return -score / 2.0


class Database:
    def __init__(self):
        self.inv = {}          # word -> list of KeyFrame (the inverted file)
        self.mnNumberOfKFs = 0

    def add(self, kf):
        self.mnNumberOfKFs += 1
        for w in kf.ids:
            self.inv.setdefault(w, []).append(kf)

    def erase(self, kf):
        if self.mnNumberOfKFs > 0:
            self.mnNumberOfKFs -= 1
        for w in kf.ids:
            lst = self.inv.get(w, [])
            for k, x in enumerate(lst):
                if x is kf:
                    del lst[k]
                    break

    def clear(self):
        self.inv = {}

    def size(self):
        return self.mnNumberOfKFs

    def empty(self):
        return self.mnNumberOfKFs == 0

    def DetectLoopCandidates(self, pKF, minScore, connected, neighbours):
        """connected: set of KeyFrame (GetConnectedKeyFrames()); neighbours(kf) -> GetBestCovisibilityKeyFrames(10) now.
        returns (candidates, lScoreAndMatch)"""
        minScore = F32(minScore)
        shared = []
        for w in pKF.ids:
            for kfi in self.inv.get(w, []):
                if kfi.mnLoopQuery != pKF.mnId:
                    kfi.mnLoopWords = 0
                    if kfi not in connected:
                        kfi.mnLoopQuery = pKF.mnId
                        shared.append(kfi)
                kfi.mnLoopWords += 1
        if not shared:
            return [], []
        maxCommonWords = 0
        for kfi in shared:
            if kfi.mnLoopWords > maxCommonWords:
                maxCommonWords = kfi.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        scored = []
        for kfi in shared:
            if kfi.mnLoopWords > minCommonWords:
                si = F32(l1_score(pKF.bow, kfi.bow))
                kfi.mLoopScore = si
                if si >= minScore:
                    scored.append((si, kfi))
        if not scored:
            return [], []
        acc_list = []
        bestAccScore = minScore
        for si, kfi in scored:
            bestScore = si
            accScore = si
            pBestKF = kfi
            for kf2 in neighbours(kfi):
                if kf2.mnLoopQuery == pKF.mnId and kf2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + kf2.mLoopScore)
                    if kf2.mLoopScore > bestScore:
                        pBestKF = kf2
                        bestScore = kf2.mLoopScore
            acc_list.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return _retain(acc_list, bestAccScore), scored

    def DetectRelocalizationCandidates(self, F, neighbours):
        """F: object with mnId and ids / vals (mBowVec)"""
        shared = []
        for w in F.ids:
            for kfi in self.inv.get(w, []):
                if kfi.mnRelocQuery != F.mnId:
                    kfi.mnRelocWords = 0
                    kfi.mnRelocQuery = F.mnId
                    shared.append(kfi)
                kfi.mnRelocWords += 1
        if not shared:
            return [], []
        maxCommonWords = 0
        for kfi in shared:
            if kfi.mnRelocWords > maxCommonWords:
                maxCommonWords = kfi.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        scored = []
        for kfi in shared:
            if kfi.mnRelocWords > minCommonWords:
                si = F32(l1_score(F.bow, kfi.bow))
                kfi.mRelocScore = si
                scored.append((si, kfi))
        if not scored:
            return [], []
        acc_list = []
        bestAccScore = F32(0.0)
        for si, kfi in scored:
            bestScore = si
            accScore = bestScore
            pBestKF = kfi
            for kf2 in neighbours(kfi):
                if kf2.mnRelocQuery != F.mnId:
                    continue
                accScore = F32(accScore + kf2.mRelocScore)
                if kf2.mRelocScore > bestScore:
                    pBestKF = kf2
                    bestScore = kf2.mRelocScore
            acc_list.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return _retain(acc_list, bestAccScore), scored


def _retain(acc_list, bestAccScore):
    minScoreToRetain = F32(0.75) * F32(bestAccScore)
    seen, out = set(), []
    for acc, kf in acc_list:
        if acc > minScoreToRetain and id(kf) not in seen:
            out.append(kf)
            seen.add(id(kf))
    return out


class Query:
    """a Frame for DetectRelocalizationCandidates"""

    def __init__(self, mnId, ids, vals):
        self.mnId = mnId
        self.ids = [int(i) for i in ids]
        self.vals = [float(v) for v in vals]

    @property
    def bow(self):
        return self.ids, self.vals


def min_score(kf, covisible):
    """LoopClosing::DetectLoop / MultiMapper::DetectLoop's minScore over the covisible keyframes (the bad ones left out)"""
    m = F32(1.0)
    for k in covisible:
        s = F32(l1_score(kf.bow, k.bow))
        if s < m:
            m = s
    return m


def random_bow(rng, pool_words, n_words, nw):
    """a BowVector of about nw words: most from the place's pool, some from anywhere; values L1-normalised (TF-IDF, L1)"""
    k_place = min(len(pool_words), int(nw * 0.8))
    w = set(rng.choice(pool_words, k_place, replace=False).tolist())
    w |= set(rng.integers(0, n_words, nw - k_place).tolist())
    ids = np.array(sorted(w), np.uint32)
    vals = rng.uniform(0.05, 3.0, ids.shape[0])
    vals = vals / vals.sum()
    return ids, vals.astype(np.float64)


def make_scene(rng, n_kf, nw=60, n_words=None, places=None, k=10, L=3):
    """n_kf keyframes spread over places (keyframes of one place share many words); returns dict(n_words, bows, place,
    covis) -- covis[i]: up to 10 keyframes of the same place, most shared words first (ties: lower slot)"""
    if n_words is None:
        voc = make_vocab(rng, k, L)
        n_words = int(voc["is_leaf"].sum())
    places = places or max(2, n_kf // 8)
    place_words = [rng.choice(n_words, min(n_words, 2 * nw), replace=False) for _ in range(places)]
    place = rng.integers(0, places, n_kf)
    bows = [random_bow(rng, place_words[place[i]], n_words, nw) for i in range(n_kf)]
    sets = [set(b[0].tolist()) for b in bows]
    by_place = {}
    for i in range(n_kf):
        by_place.setdefault(int(place[i]), []).append(i)
    covis = []
    for i in range(n_kf):
        mates = [j for j in by_place[int(place[i])] if j != i]
        if len(mates) > 40:
            mates = rng.choice(mates, 40, replace=False).tolist()
        mates.sort(key=lambda j: (-len(sets[i] & sets[j]), j))
        covis.append(mates[:10])
    return dict(n_words=n_words, bows=bows, place=place, covis=covis, place_words=place_words, nw=nw)


def query_bow(rng, scene, place=None):
    """a new frame's BowVector seen from one of the scene's places"""
    if place is None:
        place = int(rng.integers(0, len(scene["place_words"])))
    return random_bow(rng, scene["place_words"][place], scene["n_words"], scene["nw"])
