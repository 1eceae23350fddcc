// pgo_device.h -- device code of the pose graph's residual functor, shared by the kernels that evaluate it: the solver's
// linearisation (pgo.hip), the candidate-edge test (pgo_cov.hip) and the relative-pose covariances of a bundle
// adjustment (ba_cov.hip).  Forward-mode dual numbers with 12 partials (D12: what ceres::AutoDiffCostFunction<., 6, 7, 7>
// followed by the SE3 plus-Jacobian computes), quaternion helpers, Sophus' SE3 log, the residual
//     r = log(T_w_c^-1 * T_w_n) - upsilon_omega                  (PoseGraphRelativePoseCostFunctor, reprojection.h:107-126)
// and the seed of a pose's tangent T * exp(delta) (local_parameterization_se3.hpp:43-63).
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct D12 {
  double v;
  double d[12];
};
__device__ __forceinline__ D12 mk(double x) {
  D12 r;
  r.v = x;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = 0.0;
  return r;
}
__device__ __forceinline__ D12 operator+(const D12& a, const D12& b) {
  D12 r;
  r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = a.d[i] + b.d[i];
  return r;
}
__device__ __forceinline__ D12 operator-(const D12& a, const D12& b) {
  D12 r;
  r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = a.d[i] - b.d[i];
  return r;
}
__device__ __forceinline__ D12 operator-(const D12& a) {
  D12 r;
  r.v = -a.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = -a.d[i];
  return r;
}
__device__ __forceinline__ D12 operator*(const D12& a, const D12& b) {
  D12 r;
  r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
__device__ __forceinline__ D12 operator/(const D12& a, const D12& b) {
  D12 r;
  const double inv = 1.0 / b.v;
  r.v = a.v * inv;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}
__device__ __forceinline__ D12 dsqrt(const D12& a) {
  D12 r;
  r.v = sqrt(a.v);
  const double k = 0.5 / r.v;
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = a.d[i] * k;
  return r;
}
__device__ __forceinline__ D12 datan2(const D12& y, const D12& x) {
  D12 r;
  r.v = atan2(y.v, x.v);
  const double den = 1.0 / (x.v * x.v + y.v * y.v);
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = (x.v * y.d[i] - y.v * x.d[i]) * den;
  return r;
}
__device__ __forceinline__ D12 dsin(const D12& a) {
  D12 r;
  r.v = sin(a.v);
  const double c = cos(a.v);
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = c * a.d[i];
  return r;
}
__device__ __forceinline__ D12 dcos(const D12& a) {
  D12 r;
  r.v = cos(a.v);
  const double s = -sin(a.v);
#pragma unroll
  for (int i = 0; i < 12; i++) r.d[i] = s * a.d[i];
  return r;
}
__device__ __forceinline__ double dsqrt(double a) { return sqrt(a); }
__device__ __forceinline__ double datan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ double dsin(double a) { return sin(a); }
__device__ __forceinline__ double dcos(double a) { return cos(a); }
__device__ __forceinline__ double val(double a) { return a; }
__device__ __forceinline__ double val(const D12& a) { return a.v; }
__device__ __forceinline__ double lift(double, double x) { return x; }
__device__ __forceinline__ D12 lift(const D12&, double x) { return mk(x); }

template <class T>
__device__ void qmul(const T* a, const T* b, T* o) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
template <class T>
__device__ void qrot(const T* q, const T* p, T* o) {
  T uv[3] = {q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]};
  for (int i = 0; i < 3; i++) uv[i] = uv[i] + uv[i];
  const T c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; i++) o[i] = p[i] + q[3] * uv[i] + c[i];
}

// Sophus::SE3::log of (q, t): out = (upsilon, omega)   (so3.hpp logAndTheta, se3.hpp log)
template <class T>
__device__ void se3_log(const T* q, const T* t, T* out) {
  const T sq_n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
  const T w = q[3];
  T two_atan, c;
  if (val(sq_n) < 1e-20) {
    two_atan = lift(w, 2.0) / w - lift(w, 2.0 / 3.0) * sq_n / (w * w * w);
    c = lift(w, 1.0 / 12.0);
  } else {
    const T n = dsqrt(sq_n);
    const T half = val(w) < 0 ? datan2(-n, -w) : datan2(n, w);
    two_atan = lift(w, 2.0) * half / n;
    const T theta = two_atan * n;
    if (fabs(val(theta)) < 1e-6) {
      c = lift(w, 1.0 / 12.0);
    } else {
      const T ht = lift(w, 0.5) * theta;
      c = (lift(w, 1.0) - theta * dcos(ht) / (lift(w, 2.0) * dsin(ht))) / (theta * theta);
    }
  }
  const T om[3] = {two_atan * q[0], two_atan * q[1], two_atan * q[2]};
  const T a[3] = {om[1] * t[2] - om[2] * t[1], om[2] * t[0] - om[0] * t[2], om[0] * t[1] - om[1] * t[0]};
  const T b[3] = {om[1] * a[2] - om[2] * a[1], om[2] * a[0] - om[0] * a[2], om[0] * a[1] - om[1] * a[0]};
  for (int i = 0; i < 3; i++) {
    out[i] = t[i] - lift(w, 0.5) * a[i] + c * b[i];
    out[3 + i] = om[i];
  }
}

template <class T>
__device__ void edge_residual(const T* qc, const T* tc, const T* qn, const T* tn, const double* meas, T* r) {
  const T qci[4] = {-qc[0], -qc[1], -qc[2], qc[3]};
  T q[4], dt[3], t[3];
  qmul(qci, qn, q);
  for (int i = 0; i < 3; i++) dt[i] = tn[i] - tc[i];
  qrot(qci, dt, t);
  T lg[6];
  se3_log(q, t, lg);
  for (int i = 0; i < 6; i++) r[i] = lg[i] - lift(q[3], meas[i]);
}

// T exp(delta) to first order in dual arithmetic: q' = q (x) (omega / 2, 1), t' = t + R upsilon
inline __device__ void seed_pose(const double* p7, int first, D12* q, D12* t) {
  for (int i = 0; i < 4; i++) q[i] = mk(p7[i]);
  for (int i = 0; i < 3; i++) t[i] = mk(p7[4 + i]);
  for (int k = 0; k < 3; k++) {
    double e[3] = {0, 0, 0}, re[3];
    e[k] = 1.0;
    qrot(p7, e, re);
    for (int i = 0; i < 3; i++) t[i].d[first + k] = re[i];
    const double w[4] = {0.5 * e[0], 0.5 * e[1], 0.5 * e[2], 0.0};
    double qq[4];
    qmul(p7, w, qq);
    for (int i = 0; i < 4; i++) q[i].d[first + 3 + k] = qq[i];
  }
}

}  // namespace
