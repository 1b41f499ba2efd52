// orbx_streammatch.inc -- extractor, part 6 of 7: the stream matcher (every frame against the previous frame of its stream) on
// the result sets: its launches, the roll of the previous-frame slot, the match downloads.

// ------------------------------------------------------------------ stream matching
static orbm::MatchIO slots_io(orbx_handle* h, int set)
{
    orbm::MatchIO io;
    io.desc = r_desc(h, set); io.descPitch = (int64_t)h->maxKp * 32;
    if (h->fuseExpand) { io.ang = (const float*)(r_xdesc(h, set) + h->xAngOff); io.angStride = 1; io.angPitch = h->xPitch / 4; }   // k_orient_desc's compact copy
    else { io.ang = &((const float*)r_kps(h, set))[3]; io.angStride = 7; io.angPitch = (int64_t)h->maxKp * 7; }
    io.count = r_count(h, set);
    return io;
}

// last frame of the batch in `set` becomes the stream's previous frame: slot 0 of the set the next extraction fills
static int roll_prev_on(orbx_handle* h, hipStream_t s, int set)
{
    const int B = h->lastB;
    hipLaunchKernelGGL(k_roll_prev, dim3(16), dim3(256), 0, s, (const uint32_t*)(r_kps(h, set) + (size_t)B * h->maxKp),
                       (const uint32_t*)(r_desc(h, set) + (size_t)B * h->maxKp * 32), (const int32_t*)(r_count(h, set) + B),
                       (uint32_t*)r_kps(h, set ^ 1), (uint32_t*)r_desc(h, set ^ 1), r_count(h, set ^ 1),
                       h->fuseExpand ? (const uint4*)(r_xdesc(h, set) + (size_t)B * h->xPitch) : (const uint4*)nullptr, (uint4*)r_xdesc(h, set ^ 1), (int)(h->xAngOff / 16));
    HIPCHK(hipEventRecord(h->evMatch[set], s));
    HIPCHK(hipGetLastError());
    h->matchPending[set] = true;
    h->matchStream[set] = s;
    return ORBX_OK;
}

// the kernels of the stream matcher for the B frames of result set `set` (no waits, no roll)
static void match_kernels(orbx_handle* h, hipStream_t s, int set, int B, float nnratio, int th_low, int check_ori)
{
    orbm::MatchIO io = slots_io(h, set);
    int32_t* const d_match = h->d_match + (size_t)set * h->maxB * h->maxKp;  // one table per result set: the host path's
    int32_t* const d_nmatch = h->d_nmatch + (size_t)set * h->maxB;           // download of batch n-1 runs beside batch n
    h->matchSet = set;
    h->prof.begin(P_MATCH_BEST2, s);
    bool fused = false;
    // slots 0..B expanded to +-32 bytes, then the Hamming scan as an int8 MFMA product (train slot f, query slot f+1)
    // with the acceptance rule in its epilogue
    const orbm::AcceptArgs aa = {io, io, 1, 0, nnratio, th_low, check_ori, d_match, (int64_t)h->maxKp, h->d_binOf, h->d_hist};
    // the MFMA scan packs the train index into 16 bits of its key: larger frames take the popcount scan (20-bit index)
    if (h->matchPopcount || h->maxKp >= 65536) {  // the literal xor + popcount scan (lane = query, train descriptor wave-uniform): what > 65 535 features per frame take, and the form the matrix-core scan is tested against
        hipLaunchKernelGGL(orbm::k_match_best2, dim3((h->maxKp + 255) / 256, B, kMatchChunks), dim3(256), 0, s, io, io, 1, 0,
                           kMatchChunks, h->d_partial, (int64_t)h->maxKp);
        hipLaunchKernelGGL(orbm::k_match_accept, dim3((h->maxKp + 255) / 256, B), dim3(256), 0, s, aa, kMatchChunks,
                           (const uint2*)h->d_partial, (int64_t)h->maxKp);
    } else {
        // (the +-1 form is already there: k_orient_desc wrote slots 1 .. B beside the descriptors, k_roll_prev moved slot 0)
        const int nqb = (h->maxKp + orbm::kMfmaRowsPerBlock - 1) / orbm::kMfmaRowsPerBlock;
        // few frames (the one-frame-per-call entry): cut the train side into chunks so that the scan fills more than B * nqb CUs
        int chunks = 1;
        while (chunks < 8 && (size_t)B * nqb * chunks < 64 && (size_t)B * chunks * 2 <= h->partialSlots) chunks *= 2;
        hipLaunchKernelGGL(orbm::k_match_mfma, dim3(8 * ((B + 7) / 8) * nqb, chunks), dim3(orbm::kMfmaThreads), orbm::kMfmaLdsBytes, s, (const uint8_t*)r_xdesc(h, set), h->xPitch, aa, nqb, B,
                           h->d_partial, (int64_t)h->maxKp);
        fused = chunks > 1;
        if (fused)  // merge + acceptance + histogram + pruning of a frame in one workgroup
            hipLaunchKernelGGL(orbm::k_match_accept_prune, dim3(B), dim3(1024), 0, s, aa, chunks, (const uint2*)h->d_partial,
                               (int64_t)h->maxKp, d_nmatch);
    }
    h->prof.end(s);
    if (!fused) {
        h->prof.begin(P_MATCH_PRUNE, s);
        hipLaunchKernelGGL(orbm::k_match_prune, dim3(B), dim3(256), 0, s, io, 1, check_ori, d_match, (int64_t)h->maxKp,
                           h->d_binOf, h->d_hist, d_nmatch);
        h->prof.end(s);
    }
}

// the matching of the last extracted batch on stream s; roll = false leaves the roll of the previous-frame slot to the
// caller (the latency path puts the result kernel in front of it)
static int match_prev_on(orbx_handle* h, hipStream_t s, float nnratio, int th_low, int check_ori, bool roll)
{
    int rc;
    const int B = h->lastB;
    if (B < 1) return fail(ORBX_E_INVALID, "no extracted batch to match");
    const int set = h->curSet;
    // what this stream does not already follow: the batch's descriptors, the previous batch's roll into slot 0 of this
    // set, the download that last read this set's tables
    if (!(h->lastParts == 1 && h->prevSplit == 1 && !h->serial && s == h->streamP[0])) {
        if ((rc = flush_part_event(h))) return rc;
        for (int p = 0; p < h->lastParts; p++) HIPCHK(hipStreamWaitEvent(s, h->evPart[p], 0));
    }
    if (h->matchPending[set ^ 1] && h->matchStream[set ^ 1] != s) HIPCHK(hipStreamWaitEvent(s, h->evMatch[set ^ 1], 0));
    if (h->evOutOfSet[set] && h->outStream[set] != s) HIPCHK(hipStreamWaitEvent(s, h->evOutOfSet[set], 0));
    match_kernels(h, s, set, B, nnratio, th_low, check_ori);
    HIPCHK(hipGetLastError());
    if (!roll) return ORBX_OK;
    HIPCHK(hipEventRecord(h->evMatched[set], s));  // the tables are final: the host path's download need not wait for the roll
    if ((rc = roll_prev_on(h, s, set))) return rc;
    return ORBX_OK;
}

extern "C" int orbx_match_prev_batch_device(orbx_t* h, float nnratio, int th_low, int check_ori)
{
    int rc = check_device(h);
    if (rc) return rc;
    // matching runs on its own stream so that the next batch's pyramid/FAST can start beside it
    return match_prev_on(h, h->serial || !h->stream3 ? h->stream : h->stream3, nnratio, th_low, check_ori, true);
}

extern "C" int orbx_device_matches(orbx_t* h, int32_t** d_match, int32_t** d_nmatch)
{
    int rc = check_device(h);
    if (rc) return rc;
    if (d_match) *d_match = h->d_match + (size_t)h->matchSet * h->maxB * h->maxKp;
    if (d_nmatch) *d_nmatch = h->d_nmatch + (size_t)h->matchSet * h->maxB;
    return ORBX_OK;
}

extern "C" int orbx_download_matches(orbx_t* h, int frame, int32_t* match, int cap, int* nmatch)
{
    int rc = orbx_sync(h);
    if (rc) return rc;
    if (frame < 0 || frame >= h->lastB) return fail(ORBX_E_INVALID, "frame %d not in the last batch", frame);
    int32_t n = 0, nm = 0;
    HIPCHK(hipMemcpy(&n, r_count(h, h->curSet) + 1 + frame, sizeof n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&nm, h->d_nmatch + (size_t)h->matchSet * h->maxB + frame, sizeof nm, hipMemcpyDeviceToHost));
    if (nmatch) *nmatch = nm;
    if (n > cap) return fail(ORBX_E_CAPACITY, "%d queries, caller capacity %d", n, cap);
    if (match && n > 0) HIPCHK(hipMemcpy(match, h->d_match + ((size_t)h->matchSet * h->maxB + frame) * h->maxKp, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ORBX_OK;
}
