// orbx_geometry.inc -- extractor, part 2 of 7: the per-instance tables of the reference constructor, the level / cell / resize
// geometry of a frame shape (host side only), the LDS footprints of the launches, the table queries.

// ------------------------------------------------------------------ tables, ref :410-470
static int init_tables(orbx_handle* h)
{
    const OrbxParams& p = h->prm;
    if (p.nlevels < 1 || p.nlevels > ORBX_MAXL || p.nfeatures < 1 || !(p.scaleFactor > 1.0f))
        return fail(ORBX_E_INVALID, "bad ORBextractor parameters");
    const int L = p.nlevels;
    h->nlevels = L;
    const double scaleFactor = (double)p.scaleFactor;  // member is double (ORBextractor.h:93)
    h->mvScaleFactor[0] = 1.0f;
    h->mvLevelSigma2[0] = 1.0f;
    for (int i = 1; i < L; i++) {
        h->mvScaleFactor[i] = (float)((double)h->mvScaleFactor[i - 1] * scaleFactor);
        h->mvLevelSigma2[i] = h->mvScaleFactor[i] * h->mvScaleFactor[i];
    }
    for (int i = 0; i < L; i++) {
        h->mvInvScaleFactor[i] = 1.0f / h->mvScaleFactor[i];
        h->mvInvLevelSigma2[i] = 1.0f / h->mvLevelSigma2[i];
    }
    const float factor = (float)(1.0 / scaleFactor);
    float nDesired = (float)p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
        h->mnFeaturesPerLevel[l] = cv_round(nDesired);
        sum += h->mnFeaturesPerLevel[l];
        nDesired *= factor;
    }
    h->mnFeaturesPerLevel[L - 1] = std::max(p.nfeatures - sum, 0);

    int v, v0;
    const int vmax = (int)std::floor((double)((float)kHalfPatch * std::sqrt(2.f) / 2 + 1));
    const int vmin = (int)std::ceil((double)((float)kHalfPatch * std::sqrt(2.f) / 2));
    const double hp2 = kHalfPatch * kHalfPatch;
    for (v = 0; v < 16; v++) h->umax[v] = 0;
    for (v = 0; v <= vmax; ++v) h->umax[v] = cv_round(std::sqrt(hp2 - v * v));
    for (v = kHalfPatch, v0 = 0; v >= vmin; --v) {
        while (h->umax[v0] == h->umax[v0 + 1]) ++v0;
        h->umax[v] = v0;
        ++v0;
    }
    return ORBX_OK;
}

// geometry for a frame shape; fills geom/cells/tables (host side only)
struct HostGeom {
    Geom g;
    std::vector<Cell> cells;
    std::vector<short4> tabs;          // all x/y tables back to back
    int xoff[ORBX_MAXL], yoff[ORBX_MAXL];
    int tileStrideDw, tileRows, fastListCap, tileRows0, fastListCap0, fastSmapPitch, fastSmapPitch0, nodeCap;
    BlurTiles bt;
    BlurRuns br;
    KpBlocks kb;
    int kbTotal;
    std::vector<PyrRange> pyrRanges;   // [block][level]
    int pyrBlocks, pyrBufA, pyrBufB, pyrTabCap;
    bool pyrFused;
};

// k_pyramid's LDS: the two level buffers (words) and the coefficient tables of one level
static inline size_t pyr_lds_bytes(int bufA, int bufB, int tabCap) { return ((size_t)bufA + bufB) * 4 + (size_t)tabCap * 16; }

// k_orient_desc's tables as its four-keypoint form builds them in every workgroup (thread i of 256): test i of the sampling
// pattern as floats, and for item i = (row i >> 3, dword i & 7) of the IC_Angle patch the byte weights u + 16 and the flags of
// the bytes inside the disc, |u| <= umax[|v|] (v = row - 15; row 31 is loaded and carries none)
static const int8_t kPatternHost[1024] = {
#include "brief_pattern.inc"
};
static void build_orient_tables(const int umax[16], OrientTables& t)
{
    for (int i = 0; i < 256; i++) {
        t.spat[i] = make_float4((float)kPatternHost[4 * i], (float)kPatternHost[4 * i + 1], (float)kPatternHost[4 * i + 2], (float)kPatternHost[4 * i + 3]);
        const int v = (i >> 3) - kHalfPatch, u0 = 4 * (i & 7) - 16;
        const int d = i < 248 ? umax[(v < 0 ? -v : v) & 15] : -1;
        uint32_t wu = 0, w1 = 0;
        for (int j = 0; j < 4; j++) {
            const int u = u0 + j;
            if (u >= -d && u <= d) { wu |= (uint32_t)(u + 16) << (8 * j); w1 |= 1u << (8 * j); }
        }
        t.swu[i] = wu; t.sw1[i] = w1;
    }
}

static int build_geometry(const orbx_handle* h, int w, int h0, HostGeom& out)
{
    Geom& g = out.g;
    memset(&g, 0, sizeof g);
    g.nlevels = h->nlevels;
    g.w0 = w; g.h0 = h0;
    g.iniTh = h->prm.iniThFAST; g.minTh = h->prm.minThFAST;
    memcpy(g.umax, h->umax, sizeof g.umax);
    if (w > 8191 || h0 > 8191) return fail(ORBX_E_UNSUPPORTED, "frame larger than 8191 px");
    out.cells.clear();
    out.tabs.clear();
    int pyrOff = 0, blurOff = 0, candOff = 0, keptOff = 0, maxRoiW = 8, maxRoiH = 8, maxRoiW0 = 8, maxRoiH0 = 8, nodeCap = 16, maxCells = 1;
    for (int l = 0; l < g.nlevels; l++) {
        LevelGeom& L = g.lv[l];
        const float scale = h->mvInvScaleFactor[l];
        L.w = cv_round((double)((float)w * scale));   // :1111-1112
        L.h = cv_round((double)((float)h0 * scale));
        if (L.w < 1 || L.h < 1) return fail(ORBX_E_UNSUPPORTED, "pyramid level %d is empty", l);
        L.stride = align_up(L.w, 64);
        L.pyrOff = pyrOff;
        if (l > 0) pyrOff += align_up(L.stride * L.h, 256);
        L.blurStride = align_up(L.w, 64);
        L.blurOff = blurOff;
        blurOff += align_up(L.blurStride * L.h, 256);
        L.scale = h->mvScaleFactor[l];
        L.kpSize = (float)(int)((float)kPatchSize * h->mvScaleFactor[l]);  // :837
        L.nFeat = h->mnFeaturesPerLevel[l];

        // FAST window and cell grid, :773-787
        const int minBX = kMinBorder, minBY = kMinBorder;
        const int maxBX = L.w - kEdgeThreshold + 3, maxBY = L.h - kEdgeThreshold + 3;
        L.winW = maxBX - minBX; L.winH = maxBY - minBY;
        const float W = 30;
        const float width = (float)(maxBX - minBX), height = (float)(maxBY - minBY);
        L.nCols = width > 0 ? (int)(width / W) : 0;
        L.nRows = height > 0 ? (int)(height / W) : 0;
        L.cellBase = (int)out.cells.size();
        L.nCells = 0;
        int candCap = 0;
        if (L.nCols >= 1 && L.nRows >= 1) {
            L.wCell = (int)std::ceil((double)(width / L.nCols));
            L.hCell = (int)std::ceil((double)(height / L.nRows));
            uint32_t seq = 0;
            for (int i = 0; i < L.nRows; i++) {  // :789-806
                const float iniY = (float)(minBY + i * L.hCell);
                float maxY = iniY + L.hCell + 6;
                if (iniY >= maxBY - 3) continue;
                if (maxY > maxBY) maxY = (float)maxBY;
                for (int j = 0; j < L.nCols; j++) {
                    const float iniX = (float)(minBX + j * L.wCell);
                    float maxX = iniX + L.wCell + 6;
                    if (iniX >= maxBX - 6) continue;
                    if (maxX > maxBX) maxX = (float)maxBX;
                    Cell c;
                    c.level = (uint16_t)l;
                    c.x0 = (uint16_t)(int)iniX; c.y0 = (uint16_t)(int)iniY;
                    c.w = (uint16_t)((int)maxX - (int)iniX); c.h = (uint16_t)((int)maxY - (int)iniY);
                    c.ci = (uint16_t)i; c.cj = (uint16_t)j;
                    c.seq = seq++;
                    c.candOff = (uint32_t)candCap;
                    if (c.w < 7 || c.h < 7) continue;  // cv::FAST finds nothing in such a ROI
                    if (c.w > 127 || c.h > 127 || c.seq >= 65536u)
                        return fail(ORBX_E_UNSUPPORTED, "cell geometry out of range");
                    out.cells.push_back(c);
                    L.nCells++;
                    candCap += ((c.w - 6 + 1) / 2) * ((c.h - 6 + 1) / 2);
                    maxRoiW = std::max<int>(maxRoiW, c.w);
                    maxRoiH = std::max<int>(maxRoiH, c.h);
                    if (l == 0) { maxRoiW0 = std::max<int>(maxRoiW0, c.w); maxRoiH0 = std::max<int>(maxRoiH0, c.h); }
                }
            }
        }
        maxCells = std::max(maxCells, L.nCells);
        L.candOff = candOff;
        L.candCap = align_up(candCap + 8, 8);
        candOff += L.candCap;
        // quadtree roots, :543-545
        L.nIni = 0; L.hX = 0.f;
        if (L.winW > 0 && L.winH > 0) {
            L.nIni = (int)roundf((float)(maxBX - minBX) / (float)(maxBY - minBY));
            if (L.nIni >= 1) L.hX = (float)(maxBX - minBX) / (float)L.nIni;
            else if (L.nCells > 0)
                return fail(ORBX_E_UNSUPPORTED, "level %d: width/height < 0.5, the reference divides by zero (ORBextractor.cc:543-545)", l);
        }
        L.keptOff = keptOff;
        L.keptCap = align_up(std::max(L.nFeat + 4, 4 * L.nIni) + 4, 4);
        keptOff += L.keptCap;
        nodeCap = std::max(nodeCap, L.keptCap + 8);
    }
    g.totalCells = (int)out.cells.size();
    g.maxCellsPerLevel = maxCells;
    g.pyrFrameBytes = std::max(pyrOff, 256);
    g.blurFrameBytes = blurOff;
    g.candFrameRecs = candOff;
    g.keptFrameRecs = keptOff;
    g.maxKp = keptOff;
    out.tileStrideDw = maxRoiW + 5 <= 48 ? 12 : 20;      // k_fast<48> or k_fast<80> (tile row stride in bytes)
    if (maxRoiW + 5 > 80 || maxRoiW - 6 > 127 || maxRoiH - 6 > 127) return fail(ORBX_E_UNSUPPORTED, "cell larger than the FAST tile");
    out.tileRows = maxRoiH;
    out.fastListCap = ((maxRoiW - 6) * (maxRoiH - 6) + 63) / 64 * 64;  // compacted detection pixels
    // the level-0 launch (a third of the cells, all of one size) gets its own, smaller LDS footprint: more waves per CU
    out.tileRows0 = maxRoiH0;
    out.fastListCap0 = ((maxRoiW0 - 6) * (maxRoiH0 - 6) + 63) / 64 * 64;
    // the score map covers the detection area and a one-pixel apron, rows at its own pitch (bytes)
    out.fastSmapPitch = align_up(maxRoiW - 6 + 2, 4);
    out.fastSmapPitch0 = align_up(maxRoiW0 - 6 + 2, 4);
    out.nodeCap = align_up(std::max(nodeCap, 360), 4);  // k_distribute reads its u32 arrays as uint4, and parks its sort scratch (3201 words) in 9 * cap of them

    // cv::resize INTER_LINEAR coefficient tables (SURVEY.md A.2), levels >= 1
    for (int l = 0; l < g.nlevels; l++) { out.xoff[l] = out.yoff[l] = 0; }
    for (int l = 1; l < g.nlevels; l++) {
        const int sw = g.lv[l - 1].w, sh = g.lv[l - 1].h, dw = g.lv[l].w, dh = g.lv[l].h;
        const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
        const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
        if (scale_x == 2.0 && scale_y == 2.0)
            return fail(ORBX_E_UNSUPPORTED, "scale factor 2: cv::resize switches to INTER_AREA (not on this path)");
        out.xoff[l] = (int)out.tabs.size();
        std::vector<short4> xt(dw);
        int xmax = dw;
        for (int dx = 0; dx < dw; dx++) {
            float fx = (float)((dx + 0.5) * scale_x - 0.5);
            int sx = (int)std::floor(fx);
            fx -= sx;
            if (sx < 0) { fx = 0; sx = 0; }
            if (sx + 1 >= sw) {
                xmax = std::min(xmax, dx);
                if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
            }
            auto sat = [](float v) { long r = lrintf(v); return (short)(r > 32767 ? 32767 : (r < -32768 ? -32768 : r)); };
            xt[dx] = make_short4((short)sx, sat((1.f - fx) * 2048), sat(fx * 2048), 0);
        }
        for (int dx = 0; dx < dw; dx++) xt[dx].w = dx < xmax ? 1 : 0;
        out.tabs.insert(out.tabs.end(), xt.begin(), xt.end());
        out.yoff[l] = (int)out.tabs.size();
        for (int dy = 0; dy < dh; dy++) {
            float fy = (float)((dy + 0.5) * scale_y - 0.5);
            int sy = (int)std::floor(fy);
            fy -= sy;
            auto clip = [&](int y) { return y < 0 ? 0 : (y < sh ? y : sh - 1); };
            auto sat = [](float v) { long r = lrintf(v); return (short)(r > 32767 ? 32767 : (r < -32768 ? -32768 : r)); };
            out.tabs.push_back(make_short4((short)clip(sy), (short)clip(sy + 1), sat((1.f - fy) * 2048), sat(fy * 2048)));
        }
    }
    // blur tiles (kBlurTW x kBlurTH), the column walk's runs and orient/desc blocks (kKpPerBlock keypoints) per level
    int tb = 0, kb = 0, rb = 0;
    memset(&out.br, 0, sizeof out.br);
    for (int l = 0; l < g.nlevels; l++) {
        out.bt.base[l] = tb;
        out.bt.tilesX[l] = (g.lv[l].w + kBlurTW - 1) / kBlurTW;
        tb += out.bt.tilesX[l] * ((g.lv[l].h + kBlurTH - 1) / kBlurTH);
        // a column's steps in equal runs of at most kBlurRunSteps (the last may be shorter)
        const int steps = blur_walk_steps(g.lv[l].h), nruns = (steps + kBlurRunSteps - 1) / kBlurRunSteps;
        out.br.base[l] = rb;
        out.br.colsX[l] = out.bt.tilesX[l];
        out.br.runSteps[l] = (steps + nruns - 1) / nruns;
        rb += out.br.colsX[l] * ((steps + out.br.runSteps[l] - 1) / out.br.runSteps[l]);
        out.kb.base[l] = kb;
        kb += (g.lv[l].keptCap + kKpPerBlock - 1) / kKpPerBlock;
    }
    for (int l = g.nlevels; l <= ORBX_MAXL; l++) { out.bt.base[l] = tb; out.br.base[l] = rb; out.kb.base[l] = kb; }
    out.kbTotal = kb;

    // fused pyramid: every block owns the same fractional rectangle of each level;
    // the computed range of level l = owned range + what level l+1's computed range reads.
    // The block grid is refined until the LDS tiles fit; if the halo chain cannot fit at all
    // (scale factors near 2, huge frames) the per-level kernel is used instead.
    // A latency handle (max_batch <= 2) starts one refinement finer: 128 blocks instead of 32 for the one frame in flight
    out.pyrFused = false;
    out.pyrBlocks = 1; out.pyrBufA = out.pyrBufB = out.pyrTabCap = 4;
    // k_pyramid reads the taps of a dword group (outputs 4k .. 4k + 3, the tail repeating the level's last entry) as the 8
    // bytes from the group's first tap on and sums a pixel's two taps with an unsigned 16-bit dot: the group's last tap,
    // sx[3] + 1, lies at most 7 bytes behind sx[0] (5 at scale factors 1.1 - 1.3, 6 at 1.5, 7 at 1.9; level sizes are rounded,
    // so it is checked per level, not derived), and the coefficients are in [0, 2048] (fx in [0, 1)).  Established here,
    // once; a shape that breaks either takes the per-level kernel.
    bool pyrWindow = true;
    for (int l = 1; l < g.nlevels; l++) {
        const short4* xt = &out.tabs[out.xoff[l]];
        const int dw = g.lv[l].w;
        for (int dx = 0; dx < dw; dx++) {
            const int last = std::min(dx | 3, dw - 1);
            if ((int)(uint16_t)xt[last].x + 1 - (int)(uint16_t)xt[dx & ~3].x > 7) pyrWindow = false;
            if (xt[dx].y < 0 || xt[dx].y > 2048 || xt[dx].z < 0 || xt[dx].z > 2048) pyrWindow = false;
        }
        // (the vertical weights are multiplied as unsigned 16-bit halves)
        const short4* yt = &out.tabs[out.yoff[l]];
        for (int dy = 0; dy < g.lv[l].h; dy++)
            if (yt[dy].z < 0 || yt[dy].z > 2048 || yt[dy].w < 0 || yt[dy].w > 2048) pyrWindow = false;
    }
    const int refine0 = h->maxB <= h->latMaxB ? 1 : 0;
    for (int refine = refine0; refine < 4 && pyrWindow && !out.pyrFused; refine++) {
        const int nl = g.nlevels;
        const int top = nl - 1;
        // 4 x 6 blocks per frame (x 2^refine each way): wide tiles -- a level-1 row of 40+ dword groups keeps a wave on one or two
        // tile rows -- and two dozen workgroups per frame.  Round 2's 8 x 4 cost the 640 x 480 shape a fifth of its rate (its
        // tiles were 20 dword groups wide: k_pyramid 0.109 -> 0.058 ms per 64 frames) and 1241 x 376 1.6 %.
        int BX = 4 << refine, BY = 6 << refine;   // (other grids: docs/experiments.md, rounds 2 and 5)
        while (BX > 1 && g.lv[top].w / BX < 8) BX >>= 1;
        while (BY > 1 && g.lv[top].h / BY < 8) BY >>= 1;
        out.pyrBlocks = BX * BY;
        out.pyrRanges.assign((size_t)out.pyrBlocks * nl, PyrRange{0, 0, 0, 0, 0, 0, 0, 0});
        int maxA = 4, maxB = 4, tabCap = 4, maxRowOff = 0;
        for (int bj = 0; bj < BY; bj++)
            for (int bi = 0; bi < BX; bi++) {
                PyrRange* R = &out.pyrRanges[(size_t)(bj * BX + bi) * nl];
                int nx0 = 0, nx1 = 0, ny0 = 0, ny1 = 0;  // computed range of the level above (empty)
                for (int l = top; l >= 0; l--) {
                    const int w = g.lv[l].w, hh = g.lv[l].h;
                    // x boundaries are multiples of 4 so that every output dword has one owner
                    int ox0 = (int)((int64_t)bi * w / BX) & ~3, ox1 = bi + 1 == BX ? w : ((int)((int64_t)(bi + 1) * w / BX) & ~3);
                    int oy0 = (int)((int64_t)bj * hh / BY), oy1 = (int)((int64_t)(bj + 1) * hh / BY);
                    if (l == 0) ox0 = ox1 = oy0 = oy1 = 0;  // level 0 is the caller's frame: nothing to write
                    int cx0 = ox0, cx1 = ox1, cy0 = oy0, cy1 = oy1;
                    if (l < top && nx1 > nx0 && ny1 > ny0) {
                        const short4* xt = &out.tabs[out.xoff[l + 1]];
                        const short4* yt = &out.tabs[out.yoff[l + 1]];
                        int sx0 = 1 << 30, sx1 = -1, sy0 = 1 << 30, sy1 = -1;
                        // the kernel computes whole dword groups: cover the rounded-up range
                        const int nx1g = std::min<int>(g.lv[l + 1].w, nx0 + ((nx1 - nx0 + 3) & ~3));
                        for (int dx = nx0; dx < nx1g; dx++) {
                            const int a = (uint16_t)xt[dx].x, b = a + (xt[dx].w ? 2 : 1);
                            sx0 = std::min(sx0, a); sx1 = std::max(sx1, b);
                        }
                        for (int dy = ny0; dy < ny1; dy++) {
                            sy0 = std::min<int>(sy0, yt[dy].x); sy1 = std::max<int>(sy1, yt[dy].y + 1);
                        }
                        sx1 = std::min(sx1, w); sy1 = std::min(sy1, hh);
                        if (cx1 > cx0 && cy1 > cy0) {
                            cx0 = std::min(cx0, sx0); cx1 = std::max(cx1, sx1);
                            cy0 = std::min(cy0, sy0); cy1 = std::max(cy1, sy1);
                        } else { cx0 = sx0; cx1 = sx1; cy0 = sy0; cy1 = sy1; }
                    }
                    cx0 &= ~3;  // dword-aligned tile origin
                    R[l] = PyrRange{(int16_t)ox0, (int16_t)ox1, (int16_t)oy0, (int16_t)oy1,
                                    (int16_t)cx0, (int16_t)cx1, (int16_t)cy0, (int16_t)cy1};
                    if (cx1 > cx0 && cy1 > cy0) {
                        const int rowBytes = (cx1 - cx0 + 3) & ~3;
                        int rows = cy1 - cy0;
                        // the kernel stages the next level's source rows as 16-bit byte offsets from this range's first row
                        if (l < top) maxRowOff = std::max(maxRowOff, rowBytes * (rows - 1));
                        if (l == 0 && ny1 > ny0) {
                            // the kernel stages level 0 in kPyrStrips strips: the rows the strip's level-1 rows read
                            // (same split as k_pyramid: rows [chh * s / n, chh * (s + 1) / n) of level 1's computed range)
                            const short4* yt = &out.tabs[out.yoff[1]];
                            const int chh1 = ny1 - ny0;
                            rows = 0;
                            for (int sidx = 0; sidx < kPyrStrips; sidx++) {
                                const int ya = (int)((int64_t)chh1 * sidx / kPyrStrips), yb = (int)((int64_t)chh1 * (sidx + 1) / kPyrStrips);
                                if (yb > ya) rows = std::max(rows, std::min<int>(yt[ny0 + yb - 1].y + 1, cy1) - (int)yt[ny0 + ya].x);
                            }
                        }
                        // four spare words: the next level's 8-byte window (and its aligned three-dword form) starts at a tap
                        // inside a row, below byte rowBytes, and so ends at most 11 bytes behind the last row
                        const int words = rowBytes / 4 * rows + 4;
                        if (l & 1) maxB = std::max(maxB, words); else maxA = std::max(maxA, words);
                        if (l > 0) tabCap = std::max(tabCap, std::max(rowBytes, cy1 - cy0));
                    }
                    nx0 = cx0; nx1 = cx1; ny0 = cy0; ny1 = cy1;
                }
            }
        out.pyrBufA = maxA; out.pyrBufB = maxB; out.pyrTabCap = (tabCap + 3) & ~3;
        const size_t pl = pyr_lds_bytes(maxA, maxB, out.pyrTabCap);
        out.pyrFused = (pl <= 64 * 1024 || (refine == 3 && pl <= 156 * 1024)) && maxRowOff < 65536;
    }
    return ORBX_OK;
}

// ------------------------------------------------------------------ LDS footprints of the launches
// k_distribute's dynamic LDS -- and its global scratch region per (frame, level) where that does not fit (configure_shape)
static size_t dist_lds_bytes(int cap, int maxCells) { return (size_t)(19 * cap + 8 + 2 * (maxCells + 1)) * 4; }
// k_fast's LDS: the ROI tile, the score map (detection area + apron), the candidate list
static inline size_t fast_lds_bytes(int rows, int strideDw, int smapPitch, int listCap)
{
    return (size_t)(rows * strideDw + 4) * 4 + (size_t)align_up((rows - 4) * smapPitch, 8) + (size_t)listCap * 2;
}

// ------------------------------------------------------------------ table queries
extern "C" int orbx_levels(const orbx_t* h) { return h ? h->nlevels : 0; }
extern "C" float orbx_scale_factor(const orbx_t* h) { return h ? (float)(double)h->prm.scaleFactor : 0.f; }
extern "C" int orbx_scale_tables(const orbx_t* h, float* s, float* is, float* s2, float* is2)
{
    if (!h) return fail(ORBX_E_INVALID, "null handle");
    for (int i = 0; i < h->nlevels; i++) {
        if (s) s[i] = h->mvScaleFactor[i];
        if (is) is[i] = h->mvInvScaleFactor[i];
        if (s2) s2[i] = h->mvLevelSigma2[i];
        if (is2) is2[i] = h->mvInvLevelSigma2[i];
    }
    return ORBX_OK;
}
extern "C" int orbx_features_per_level(const orbx_t* h, int32_t* out)
{
    if (!h || !out) return fail(ORBX_E_INVALID, "null argument");
    for (int i = 0; i < h->nlevels; i++) out[i] = h->mnFeaturesPerLevel[i];
    return ORBX_OK;
}
extern "C" int orbx_umax(const orbx_t* h, int32_t out[16])
{
    if (!h || !out) return fail(ORBX_E_INVALID, "null argument");
    for (int i = 0; i < 16; i++) out[i] = h->umax[i];
    return ORBX_OK;
}
extern "C" int orbx_max_keypoints(const orbx_t* h)
{
    if (!h) return 0;
    if (h->device >= 0) return h->maxKp;
    HostGeom hg;
    if (h->maxW < 1 || h->maxH < 1 || build_geometry(h, h->maxW, h->maxH, hg)) return 0;
    return hg.g.maxKp + 64;
}
