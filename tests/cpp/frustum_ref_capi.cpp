// C shim over tools/frustum_ref.hpp for tests/ref_shim.py: the restatement of Frame::isInFrustum + the head of
// SearchByProjection(F, vpMapPoints, th), and of SearchByProjection(CurrentFrame, LastFrame)'s projection loop, over arrays.
#include "../../tools/frustum_ref.hpp"

using namespace frustum_ref;

static void store(const Query& q, int i, float* uvr, int8_t* lvl, float* viewcos, uint8_t* valid, uint8_t* obs, uint8_t* status)
{
    uvr[3 * i] = q.u; uvr[3 * i + 1] = q.v; uvr[3 * i + 2] = q.r;
    lvl[2 * i] = q.lvl[0]; lvl[2 * i + 1] = q.lvl[1];
    if (viewcos) viewcos[i] = q.viewCos;
    valid[i] = q.valid; obs[i] = q.obs; status[i] = q.status;
}

// pts: the pool's records by id; ids[nq] index it
extern "C" void frustum_local(const View* F, const Point* pts, const int32_t* ids, int nq, float th, const float* scaleFactors, int nlevels,
                              float logScaleFactor, float* uvr, int8_t* lvl, float* viewcos, uint8_t* valid, uint8_t* obs, uint8_t* status)
{
    for (int i = 0; i < nq; i++) store(localPoint(*F, pts[ids[i]], th, scaleFactors, nlevels, logScaleFactor), i, uvr, lvl, viewcos, valid, obs, status);
}

// ids[i]: the pool id of LastFrame feature i's MapPoint or -1; octaves[i]: LastFrame.mvKeys[i].octave
extern "C" void frustum_frame(const View* F, const Point* pts, const int32_t* ids, const int32_t* octaves, int nq, float th,
                              const float* scaleFactors, float* uvr, int8_t* lvl, uint8_t* valid, uint8_t* obs, uint8_t* status)
{
    for (int i = 0; i < nq; i++) store(framePoint(*F, ids[i] < 0 ? nullptr : &pts[ids[i]], octaves[i], th, scaleFactors), i, uvr, lvl, nullptr, valid, obs, status);
}
