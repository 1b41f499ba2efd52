// orbv_host.inc -- host side of the vocabulary (part of orbslamm_hip.hip): tree upload, the ORBvoc.txt loader, transform,
// Frame::ComputeBoW and SearchByBoW on device-resident frames.

// ------------------------------------------------------------------ vocabulary (SURVEY 8f.2)
// The list of a vocabulary's device scratch blocks (OrbmSlot's rule: one name per role, no numbers), all used under orbv_handle::mu.  SV_DESC .. SV_KEYS: a
// transform's (SV_OUT holds the results until the caller has taken them).  SV_SCORE: orbv_score's packed block (orbk_host.inc).
enum OrbvSlot { SV_DESC, SV_WORD, SV_NODE, SV_W, SV_OUT, SV_KEYS, SV_SCORE, SV_COUNT };
struct orbv_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    int k = 0, L = 0, scoring = 0, weighting = 0, nNodes = 0, nWords = 0;
    uint64_t serial = 0;             // unique per vocabulary made in this process (a frame set slot records the one that transformed it)
    std::vector<int> nodesAtLevel;   // [0 .. deepest]: how many nodes the tree has at each depth (root = 0)
    int32_t* d_childStart = nullptr; int32_t* d_childIdx = nullptr; uint8_t* d_desc = nullptr;
    int32_t* d_wordId = nullptr; double* d_weight = nullptr;
    void* d_buf[SV_COUNT] = {nullptr}; size_t d_cap[SV_COUNT] = {0};
    // ONE vocabulary serves every thread of a System (Frame::ComputeBoW on the Tracking thread, KeyFrame::ComputeBoW on
    // LocalMapping's and LoopClosing's, all through the same ORBVocabulary*): a transform owns the scratch for its duration
    std::mutex mu;
    // pinned twin of the input / output block of orbv_transform (+ 64 bytes: the flag the host polls)
    void* h_stage = nullptr; size_t h_stageCap = 0; int32_t stageSeq = 0;
    size_t aggLds[2] = {0, 0};           // dynamic LDS already granted to k_voc_aggregate<false / true>
};

static int orbv_reserve(orbv_handle* h, OrbvSlot s, size_t bytes) { return grow_device(h->d_buf[s], h->d_cap[s], bytes, 4096); }
template <class T = void> static T* slot_ptr(const orbv_handle* h, OrbvSlot s) { return (T*)h->d_buf[s]; }

extern "C" void orbv_destroy(orbv_t* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    void* ptrs[] = {h->d_childStart, h->d_childIdx, h->d_desc, h->d_wordId, h->d_weight};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (auto p : h->d_buf) if (p) (void)hipFree(p);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    delete h;
}

extern "C" int orbv_create(int device, int k, int L, int scoring, int weighting, int n,
                           const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                           const double* weight, orbv_t** out)
{
    if (!out) return fail(ORBX_E_INVALID, "null argument");
    *out = nullptr;
    // same sanity window as loadFromTextFile (:1360)
    if (k < 0 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3 || n < 0 ||
        (n && (!parent || !is_leaf || !desc || !weight)))
        return fail(ORBX_E_INVALID, "not a correct vocabulary");
    int ndev = orbx_device_count();
    if (ndev == 0) return fail(ORBX_E_NO_DEVICE, "no HIP device visible: the vocabulary transform has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(ORBX_E_INVALID, "device %d out of range", device);
    const int nNodes = n + 1;
    std::vector<int32_t> cnt(nNodes + 1, 0), childStart(nNodes + 1, 0), childIdx(std::max(n, 1)), wordId(nNodes, -1);
    std::vector<double> w(nNodes, 0.0);
    std::vector<uint8_t> d((size_t)nNodes * 32, 0);
    for (int i = 0; i < n; i++) {
        if (parent[i] < 0 || parent[i] > i) return fail(ORBX_E_INVALID, "node %d: parent %d does not precede it", i + 1, parent[i]);
        cnt[parent[i]]++;
    }
    for (int i = 0; i < nNodes; i++) childStart[i + 1] = childStart[i] + cnt[i];
    std::fill(cnt.begin(), cnt.end(), 0);
    int nWords = 0;
    for (int i = 0; i < n; i++) {
        const int nid = i + 1, pid = parent[i];
        childIdx[childStart[pid] + cnt[pid]++] = nid;     // m_nodes[pid].children.push_back(nid)
        memcpy(&d[(size_t)nid * 32], desc + (size_t)i * 32, 32);
        w[nid] = weight[i];
        if (is_leaf[i]) wordId[nid] = nWords++;
    }
    // every inner node must have children, every childless node must be a word (else the descent of :1236-1253 derails)
    for (int i = 1; i < nNodes; i++)
        if ((childStart[i + 1] == childStart[i]) != (wordId[i] >= 0)) return fail(ORBX_E_INVALID, "node %d: leaf flag and children disagree", i);
    // Device layout: the nodes RENUMBERED breadth first (root 0, then every node's children in their push_back order),
    // so that the children of node i are the consecutive nodes [first[i], first[i + 1]) -- a level of the descent is two
    // dependent loads (the range, then the children's descriptors) instead of three (range, child ids, descriptors).
    // origId maps back: the FeatureVector is keyed by the file's node ids.
    std::vector<int32_t> order(nNodes), newOf(nNodes, -1), first(nNodes + 1, 0), origId(nNodes), wordIdN(nNodes, -1);
    std::vector<double> wN(nNodes, 0.0);
    std::vector<uint8_t> dN((size_t)nNodes * 32, 0);
    {
        int head = 0, tail = 0;
        order[tail++] = 0; newOf[0] = 0;
        while (head < tail) {
            const int old = order[head];
            first[head] = tail;
            for (int c = childStart[old]; c < childStart[old + 1]; c++) { newOf[childIdx[c]] = tail; order[tail++] = childIdx[c]; }
            head++;
        }
        if (tail != nNodes) return fail(ORBX_E_INVALID, "not a tree: %d of %d nodes hang off the root", tail, nNodes);
        first[nNodes] = nNodes;
        for (int i = 0; i < nNodes; i++) {
            const int old = order[i];
            origId[i] = old; wordIdN[i] = wordId[old]; wN[i] = w[old];
            memcpy(&dN[(size_t)i * 32], &d[(size_t)old * 32], 32);
        }
    }
    static std::atomic<uint64_t> serials(0);
    orbv_handle* h = new orbv_handle();
    h->serial = ++serials;
    h->device = device; h->k = k; h->L = L; h->scoring = scoring; h->weighting = weighting; h->nNodes = nNodes; h->nWords = nWords;
    {
        std::vector<int> depth(nNodes, 0);
        h->nodesAtLevel.assign(1, 1);
        for (int i = 0; i < n; i++) {
            const int dpt = depth[i + 1] = depth[parent[i]] + 1;
            if ((int)h->nodesAtLevel.size() <= dpt) h->nodesAtLevel.resize(dpt + 1, 0);
            h->nodesAtLevel[dpt]++;
        }
    }
    HIPCHK_OR(hipSetDevice(device), orbv_destroy(h));
    HIPCHK_OR(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), orbv_destroy(h));
    HIPCHK_OR(hipMalloc(&h->d_childStart, (size_t)(nNodes + 1) * 4), orbv_destroy(h));
    HIPCHK_OR(hipMalloc(&h->d_childIdx, (size_t)nNodes * 4), orbv_destroy(h));
    HIPCHK_OR(hipMalloc(&h->d_desc, (size_t)nNodes * 32), orbv_destroy(h));
    HIPCHK_OR(hipMalloc(&h->d_wordId, (size_t)nNodes * 4), orbv_destroy(h));
    HIPCHK_OR(hipMalloc(&h->d_weight, (size_t)nNodes * 8), orbv_destroy(h));
    HIPCHK_OR(hipMemcpy(h->d_childStart, first.data(), (size_t)(nNodes + 1) * 4, hipMemcpyHostToDevice), orbv_destroy(h));
    HIPCHK_OR(hipMemcpy(h->d_childIdx, origId.data(), (size_t)nNodes * 4, hipMemcpyHostToDevice), orbv_destroy(h));   // (the slot of the old child list: now origId)
    HIPCHK_OR(hipMemcpy(h->d_desc, dN.data(), (size_t)nNodes * 32, hipMemcpyHostToDevice), orbv_destroy(h));
    HIPCHK_OR(hipMemcpy(h->d_wordId, wordIdN.data(), (size_t)nNodes * 4, hipMemcpyHostToDevice), orbv_destroy(h));
    HIPCHK_OR(hipMemcpy(h->d_weight, wN.data(), (size_t)nNodes * 8, hipMemcpyHostToDevice), orbv_destroy(h));
    *out = h;
    return ORBX_OK;
}

extern "C" int orbv_load_text(int device, const char* path, orbv_t** out)
{
    if (!path || !out) return fail(ORBX_E_INVALID, "null argument");
    std::ifstream f(path);
    if (!f.is_open()) return fail(ORBX_E_INVALID, "cannot open %s", path);
    std::string s;
    std::getline(f, s);
    std::stringstream ss(s);
    int k = -1, L = -1, n1 = -1, n2 = -1;
    ss >> k >> L >> n1 >> n2;
    if (k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3)
        return fail(ORBX_E_INVALID, "Vocabulary loading failure: This is not a correct text file!");
    std::vector<int32_t> parent; std::vector<uint8_t> leaf, desc; std::vector<double> weight;
    while (std::getline(f, s)) {
        if (s.find_first_not_of(" \t\r\n") == std::string::npos) continue;  // the reference trips over a trailing newline
        std::stringstream sn(s);
        int pid = -1, isLeaf = 0;
        sn >> pid >> isLeaf;
        parent.push_back(pid); leaf.push_back(isLeaf > 0);
        for (int i = 0; i < 32; i++) { int b = 0; sn >> b; desc.push_back((uint8_t)b); }  // FORB::fromString
        double w = 0; sn >> w; weight.push_back(w);
        if (sn.fail()) return fail(ORBX_E_INVALID, "malformed vocabulary line %zu", parent.size() + 1);
    }
    return orbv_create(device, k, L, n1, n2, (int)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data(), out);
}

// transform of n device-resident descriptors; the results stay in the handle's scratch: ONE block (VocOut) that a host
// caller takes home in one copy, counts = {words, fv nodes}
constexpr int kVocMaxFeatures = 1 << 20;   // (the sort key holds the feature index in 32 bits; a bound on the scratch, not on the algorithm)
struct VocOut {
    size_t oCnt, oOv, oOw, oFn, oFs, oFi, bytes;
    uint8_t* base;
    int32_t* cnt() const { return (int32_t*)(base + oCnt); }
    double* ov() const { return (double*)(base + oOv); }
    uint32_t* ow() const { return (uint32_t*)(base + oOw); }
    uint32_t* fn() const { return (uint32_t*)(base + oFn); }
    int32_t* fs() const { return (int32_t*)(base + oFs); }
    int32_t* fi() const { return (int32_t*)(base + oFi); }
};
static VocOut voc_out_layout(int n, uint8_t* base)
{
    auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
    VocOut o;
    o.oCnt = 0; o.oOv = 16; o.oOw = o.oOv + pad((size_t)n * 8); o.oFn = o.oOw + pad((size_t)n * 4); o.oFs = o.oFn + pad((size_t)n * 4);
    o.oFi = o.oFs + pad((size_t)(n + 1) * 4); o.bytes = o.oFi + pad((size_t)n * 4);
    o.base = base;
    return o;
}

// launches only; the caller syncs (voc_transform_device) or downloads the block behind a flag (orbv_transform)
static int voc_transform_launch(orbv_handle* h, const uint8_t* d_desc, int n, int levelsup, VocOut& out)
{
    if (n > kVocMaxFeatures) return fail(ORBX_E_UNSUPPORTED, "more than %d descriptors per transform", kVocMaxFeatures);
    int P = 2;
    while (P < n) P <<= 1;
    out = voc_out_layout(n, nullptr);
    int rc;
    if ((rc = orbv_reserve(h, SV_WORD, (size_t)n * 4)) || (rc = orbv_reserve(h, SV_NODE, (size_t)n * 4)) || (rc = orbv_reserve(h, SV_W, (size_t)n * 8)) ||
        (rc = orbv_reserve(h, SV_OUT, out.bytes))) return rc;
    out.base = slot_ptr<uint8_t>(h, SV_OUT);
    hipStream_t s = h->stream;
    orbv::VocDev v{h->d_childStart, h->d_childIdx, h->d_desc, h->d_wordId, h->d_weight, h->L, h->scoring, h->weighting};
    hipLaunchKernelGGL(orbv::k_voc_descend, dim3((n + 63) / 64), dim3(64), 0, s, v, d_desc, n, levelsup,
                       slot_ptr<uint32_t>(h, SV_WORD), slot_ptr<uint32_t>(h, SV_NODE), slot_ptr<double>(h, SV_W));
    if (P > 8192) {
        // more descriptors than the sort's keys fit a CU's LDS for: the same kernel body on a scratch block in memory
        if ((rc = orbv_reserve(h, SV_KEYS, (size_t)P * 12))) return rc;
        hipLaunchKernelGGL(orbv::k_voc_aggregate_mem, dim3(1), dim3(orbv::kAggThreads), 0, s, v, n, P, slot_ptr<const uint32_t>(h, SV_WORD),
                           slot_ptr<const uint32_t>(h, SV_NODE), slot_ptr<const double>(h, SV_W), out.ow(), out.ov(), out.fn(), out.fs(), out.fi(), out.cnt(),
                           slot_ptr<uint64_t>(h, SV_KEYS));
        HIPCHK(hipGetLastError());
        return ORBX_OK;
    }
    const bool accLds = P <= 4096;
    const size_t lds = (size_t)P * (accLds ? 36 : 12);
    auto kern = accLds ? orbv::k_voc_aggregate<true> : orbv::k_voc_aggregate<false>;
    if (lds > 48 * 1024 && lds > h->aggLds[accLds]) {
        HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        h->aggLds[accLds] = lds;
    }
    hipLaunchKernelGGL(kern, dim3(1), dim3(orbv::kAggThreads), lds, s, v, n, P, slot_ptr<const uint32_t>(h, SV_WORD),
                       slot_ptr<const uint32_t>(h, SV_NODE), slot_ptr<const double>(h, SV_W), out.ow(), out.ov(), out.fn(), out.fs(), out.fi(), out.cnt());
    HIPCHK(hipGetLastError());
    return ORBX_OK;
}

static int voc_transform_device(orbv_handle* h, const uint8_t* d_desc, int n, int levelsup, int32_t counts[2], VocOut& out)
{
    counts[0] = counts[1] = 0;
    int rc = voc_transform_launch(h, d_desc, n, levelsup, out);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(counts, out.cnt(), 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}

// One call = the descriptors up through a copy kernel from the pinned block, two launches, the whole result block down
// through a copy kernel with a flag behind it that the host polls (the pattern of orbt_host.inc's drop-in calls; until
// round 5: a pageable copy up, a stream sync, five synchronous copies down).
extern "C" int orbv_transform(orbv_t* h, const uint8_t* desc, int n, int levelsup,
                              uint32_t* word_id, double* word_value, int* n_words,
                              uint32_t* fv_node, int32_t* fv_start, int32_t* fv_idx, int* n_fv_nodes)
{
    if (!h) return fail(ORBX_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (n < 0 || (n && (!desc || !word_id || !word_value || !fv_node || !fv_idx)) || !fv_start || !n_words || !n_fv_nodes)
        return fail(ORBX_E_INVALID, "bad argument");
    *n_words = 0; *n_fv_nodes = 0; fv_start[0] = 0;
    if (h->nWords == 0 || n == 0) return ORBX_OK;  // empty(): v and fv stay cleared (:1133-1136)
    if (n > kVocMaxFeatures) return fail(ORBX_E_UNSUPPORTED, "more than %d descriptors per transform", kVocMaxFeatures);
    std::lock_guard<std::mutex> lk(h->mu);
    int rc;
    const size_t inBytes = ((size_t)n * 32 + 15) & ~(size_t)15;
    const VocOut lay = voc_out_layout(n, nullptr);
    const size_t need = inBytes + lay.bytes;
    if ((rc = grow_pinned(h->h_stage, h->h_stageCap, need, true)) || (rc = orbv_reserve(h, SV_DESC, inBytes))) return rc;
    uint8_t* hs = (uint8_t*)h->h_stage;
    hipStream_t s = h->stream;
    memcpy(hs, desc, (size_t)n * 32);
    hipLaunchKernelGGL(k_upload, dim3((unsigned)((inBytes / 16 + 255) / 256)), dim3(256), 0, s, (const uint4*)hs, slot_ptr<uint4>(h, SV_DESC), (int)(inBytes / 16));
    VocOut out;
    if ((rc = voc_transform_launch(h, slot_ptr<const uint8_t>(h, SV_DESC), n, levelsup, out))) return rc;
    volatile int32_t* flag = (volatile int32_t*)(hs + h->h_stageCap);
    const int32_t want = ++h->stageSeq;
    hipLaunchKernelGGL(k_upload, dim3((unsigned)((out.bytes / 16 + 255) / 256)), dim3(256), 0, s, (const uint4*)out.base, (uint4*)(hs + inBytes), (int)(out.bytes / 16));
    hipLaunchKernelGGL(k_raise_flag, dim3(1), dim3(64), 0, s, (int32_t*)flag, want);
    HIPCHK(hipGetLastError());
    if (!wait_flag(flag, want)) HIPCHK(hipStreamSynchronize(s));
    const VocOut ho = voc_out_layout(n, hs + inBytes);
    const int nw = ho.cnt()[0], nn = ho.cnt()[1];
    *n_words = nw; *n_fv_nodes = nn;
    if (nw) { memcpy(word_id, ho.ow(), (size_t)nw * 4); memcpy(word_value, ho.ov(), (size_t)nw * 8); }
    memcpy(fv_start, ho.fs(), (size_t)(nn + 1) * 4);
    if (nn) {
        memcpy(fv_node, ho.fn(), (size_t)nn * 4);
        const int m = fv_start[nn];
        if (m) memcpy(fv_idx, ho.fi(), (size_t)m * 4);
    }
    return ORBX_OK;
}

// ------------------------------------------------------------------ SURVEY 8(f).2+3: BoW on a device-resident Frame
// Frame::ComputeBoW (src/Frame.cc:394-402) on the frame's descriptors in HBM: the BowVector goes to the host (the
// KeyFrame database and the relocaliser read it), the FeatureVector stays with the frame for SearchByBoW.
extern "C" int orbm_frame_compute_bow(orbm_frame_t* f, orbv_t* voc, int levelsup,
                                      uint32_t* word_id, double* word_value, int* n_words)
{
    if (!f || !f->owner || !voc) return fail(ORBX_E_INVALID, "null argument");
    int rc = orbm_check(f->owner);
    if (rc) return rc;
    if (voc->device != f->owner->device) return fail(ORBX_E_INVALID, "vocabulary and frame live on different devices");
    if (!n_words || (f->n && (!word_id || !word_value))) return fail(ORBX_E_INVALID, "bad argument");
    *n_words = 0;
    f->fvNode.clear(); f->fvNodes = 0; f->hasBow = true;
    if (voc->nWords == 0 || f->n == 0) return ORBX_OK;
    if ((rc = frame_settle(f))) return rc;   // the vocabulary's kernels run on its own stream
    std::lock_guard<std::mutex> lk(voc->mu);
    int32_t counts[2];
    VocOut out;
    if ((rc = voc_transform_device(voc, f->d_desc, f->n, levelsup, counts, out))) return rc;
    *n_words = counts[0];
    if (counts[0]) {
        HIPCHK(hipMemcpy(word_id, out.ow(), (size_t)counts[0] * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(word_value, out.ov(), (size_t)counts[0] * 8, hipMemcpyDeviceToHost));
    }
    f->fvNodes = counts[1];
    f->fvNode.resize((size_t)counts[1]);
    HIPCHK(hipMemcpy(f->d_fvStart, out.fs(), (size_t)(counts[1] + 1) * 4, hipMemcpyDeviceToDevice));
    if (counts[1]) {
        HIPCHK(hipMemcpy(f->fvNode.data(), out.fn(), (size_t)counts[1] * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(f->d_fvIdx, out.fi(), (size_t)f->n * 4, hipMemcpyDeviceToDevice));
    }
    return ORBX_OK;
}

/* SearchByBoW between two device-resident frames (query = the KeyFrame / pKF1, train = the Frame / pKF2) */
extern "C" int orbm_search_by_bow_frames(orbm_t* h, orbm_frame_t* q, const uint8_t* qvalid, orbm_frame_t* t, const uint8_t* tvalid,
                                         float nnratio, int check_ori, int out_by_train, int32_t* match, int* nmatches)
{
    int rc = orbm_check(h);
    if (rc) return rc;
    if (!q || !t) return fail(ORBX_E_INVALID, "null frame");
    if ((rc = frame_usable(h, q)) || (rc = frame_usable(h, t))) return rc;
    if (!q->hasBow || !t->hasBow) return fail(ORBX_E_INVALID, "orbm_frame_compute_bow has not run on both frames");
    if (!match) return fail(ORBX_E_INVALID, "bad argument");
    const int nout = out_by_train ? t->n : q->n;
    for (int i = 0; i < nout; i++) match[i] = -1;
    if (nmatches) *nmatches = 0;
    if (q->n == 0 || t->n == 0 || q->fvNodes == 0 || t->fvNodes == 0) return ORBX_OK;
    const BowSide qs = {q->d_desc, q->d_ang, q->d_fvStart, q->d_fvIdx, q->fvNode.data(), q->fvNodes, q->n};
    const BowSide ts = {t->d_desc, t->d_ang, t->d_fvStart, t->d_fvIdx, t->fvNode.data(), t->fvNodes, t->n};
    return bow_core(h, qs, qvalid, ts, tvalid, nnratio, check_ori, out_by_train, match, nmatches);
}
