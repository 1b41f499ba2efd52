// Test infrastructure: g2o::Sim3 as Optimizer::OptimizeSim3's caller sees it (Thirdparty/g2o/g2o/types/sim3.h: rotation(),
// translation(), scale(), the (Quaterniond, Vector3d, double) constructor), with Eigen's Quaterniond and Vector3d reduced to their
// coefficient access, on top of tests/cpp/mock_slam.hpp: no g2o or Eigen is installed.  Plain data holders: nothing here
// computes what the product computes.
#pragma once

#include "mock_slam.hpp"

namespace s3mock {

template <int N> struct Vec {
    double v[N];
    Vec() { for (int i = 0; i < N; i++) v[i] = 0.0; }
    double& operator[](int i) { return v[i]; }
    const double& operator[](int i) const { return v[i]; }
};
struct Quaterniond {   // coeffs(): x y z w
    Vec<4> c;
    Quaterniond() { c[3] = 1.0; }
    Vec<4>& coeffs() { return c; }
    const Vec<4>& coeffs() const { return c; }
};
typedef Vec<3> Vector3d;

struct Sim3 {
    Sim3() : s(1.) {}
    Sim3(const Quaterniond& r_, const Vector3d& t_, double s_) : r(r_), t(t_), s(s_) { constructed++; }
    const Quaterniond& rotation() const { return r; }
    Quaterniond& rotation() { return r; }
    const Vector3d& translation() const { return t; }
    Vector3d& translation() { return t; }
    const double& scale() const { return s; }
    double& scale() { return s; }
    int constructed = 0;   // 1 on an object the drop-in assigned from its three-argument constructor
protected:
    Quaterniond r;
    Vector3d t;
    double s;
};

}  // namespace s3mock
