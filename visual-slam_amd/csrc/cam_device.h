// cam_device.h -- device restatement of the host's bearing and triangulation helpers: unproject() of the four camera
// models (include/visnav_amd/harness/camera.h, after include/visnav/camera_models.h pinhole :75-117, eucm :158-213,
// ds :246-302, kb4 :341-438) and triangulate_midpoint() (include/visnav_amd/harness/pnp.h).  Every expression is the
// host's, operand for operand and in the same association order: with -ffp-contract=off (csrc/Makefile) and
// correctly rounded f64 division and sqrt, the pinhole / eucm / ds bearings and the triangulated points are the host's
// bits.  kb4 calls sin / cos, whose device results may differ from the host libm in the last bit.
//
// Also the forward side used by guided_search.h: quat_rotate_d() and project_exact() -- camera_models.h project(),
// expression for expression.
#pragma once
#include <cmath>

#include "vsl_common.h"

namespace {

struct CamVec3 {
  double x, y, z;
};

// harness/camera.h unproject(); intr = fx fy cx cy p1..p4 (the intr8 layout of include/vslam_hip.h)
__device__ __forceinline__ CamVec3 cam_unproject(int model, const double* __restrict__ param, double u, double v) {
  const double fx = param[0], fy = param[1], cx = param[2], cy = param[3];
  const double mx = (u - cx) / fx, my = (v - cy) / fy;
  if (model == VSL_CAM_PINHOLE) {
    const double s = 1.0 / sqrt(mx * mx + my * my + 1.0);
    return {mx * s, my * s, s};
  }
  if (model == VSL_CAM_EUCM) {
    const double alpha = param[4], beta = param[5];
    const double rr = mx * mx + my * my;
    const double mz = (1.0 - beta * alpha * alpha * rr) / (alpha * sqrt(1.0 - (2.0 * alpha - 1.0) * beta * rr) + (1.0 - alpha));
    const double s = 1.0 / sqrt(mx * mx + my * my + mz * mz);
    return {mx * s, my * s, mz * s};
  }
  if (model == VSL_CAM_DS) {
    const double xi = param[4], alpha = param[5];
    const double rr = mx * mx + my * my;
    const double mz = (1.0 - alpha * alpha * rr) / (alpha * sqrt(1.0 - (2.0 * alpha - 1.0) * rr) + 1.0 - alpha);
    const double s = (mz * xi + sqrt(mz * mz + (1.0 - xi * xi) * rr)) / (mz * mz + rr);
    return {mx * s, my * s, mz * s - xi};
  }
  // kb4: five Newton steps from theta = 0 (camera_models.h:404-424)
  const double k1 = param[4], k2 = param[5], k3 = param[6], k4 = param[7];
  const double ru = sqrt(mx * mx + my * my);
  double th = 0.0;
  for (int it = 0; it < 5; it++) {
    const double t2 = th * th;
    const double f = th + k1 * th * t2 + k2 * th * t2 * t2 + k3 * th * t2 * t2 * t2 + k4 * th * t2 * t2 * t2 * t2 - ru;
    const double df = 1.0 + 3.0 * k1 * t2 + 5.0 * k2 * t2 * t2 + 7.0 * k3 * t2 * t2 * t2 + 9.0 * k4 * t2 * t2 * t2 * t2;
    th = th - f / df;
  }
  if (ru == 0.0) return {0.0, 0.0, cos(th)};
  return {sin(th) * mx / ru, sin(th) * my / ru, cos(th)};
}

__device__ __forceinline__ double cam_dot(const CamVec3& a, const CamVec3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// m * v with a row-major 3x3 m (harness/geometry.h operator*(Mat3, Vec3))
__device__ __forceinline__ CamVec3 cam_mul(const double* __restrict__ m, const CamVec3& v) {
  return {m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z};
}

// harness/pnp.h triangulate_midpoint(): f1 in frame 1, f2 in frame 2, p_1 = R_1_2 p_2 + t_1_2 (R row-major); the
// midpoint of the shortest segment between the two rays, in frame 1
__device__ __forceinline__ CamVec3 cam_triangulate_midpoint(const CamVec3& f1, const CamVec3& f2, const double* __restrict__ R_1_2,
                                                            const double* __restrict__ t_1_2) {
  const CamVec3 d1 = f1, d2 = cam_mul(R_1_2, f2);
  const CamVec3 t = {t_1_2[0], t_1_2[1], t_1_2[2]};
  const double a = cam_dot(d1, d1), b = cam_dot(d1, d2), c = cam_dot(d2, d2);
  const double e = cam_dot(d1, t), g = cam_dot(d2, t);
  const double den = a * c - b * b;
  if (fabs(den) < 1e-18) return {1e6 * d1.x, 1e6 * d1.y, 1e6 * d1.z};  // parallel rays: a far point along the ray
  const double l1 = (e * c - b * g) / den, l2 = (b * e - a * g) / den;
  const CamVec3 p1 = {l1 * d1.x, l1 * d1.y, l1 * d1.z};
  const CamVec3 p2 = {t.x + l2 * d2.x, t.y + l2 * d2.y, t.z + l2 * d2.z};
  return {0.5 * (p1.x + p2.x), 0.5 * (p1.y + p2.y), 0.5 * (p1.z + p2.z)};
}

__device__ __forceinline__ void quat_rotate_d(const double* q, const double* p, double* out) {
  double uv[3] = {q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]};
  for (int i = 0; i < 3; i++) uv[i] = uv[i] + uv[i];
  const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; i++) out[i] = p[i] + q[3] * uv[i] + c[i];
}

// camera_models.h project(), expression for expression (include/visnav/camera_models.h:75-94, :158-178,
// :246-270, :341-374)
__device__ __forceinline__ void project_exact(int model, const double* ip, double x, double y, double z, double& u,
                                              double& v) {
  const double fx = ip[0], fy = ip[1], cx = ip[2], cy = ip[3];
  if (model == VSL_CAM_PINHOLE) {
    u = fx * x / z + cx;
    v = fy * y / z + cy;
  } else if (model == VSL_CAM_EUCM) {
    const double alpha = ip[4], beta = ip[5];
    const double d = sqrt(beta * (x * x + y * y) + z * z);
    u = fx * x / (alpha * d + (1.0 - alpha) * z) + cx;
    v = fy * y / (alpha * d + (1.0 - alpha) * z) + cy;
  } else if (model == VSL_CAM_KB4) {
    const double k1 = ip[4], k2 = ip[5], k3 = ip[6], k4 = ip[7];
    const double r = sqrt(x * x + y * y);
    const double theta = atan2(r, z);
    const double d = theta + k1 * theta * theta * theta + k2 * theta * theta * theta * theta * theta +
                     k3 * theta * theta * theta * theta * theta * theta * theta +
                     k4 * theta * theta * theta * theta * theta * theta * theta * theta * theta;
    if (r == 0.0) {
      u = cx;
      v = cy;
    } else {
      u = fx * d * x / r + cx;
      v = fy * d * y / r + cy;
    }
  } else {
    const double xi = ip[4], alpha = ip[5];
    const double d1 = sqrt(x * x + y * y + z * z);
    const double d2 = sqrt(x * x + y * y + (xi * d1 + z) * (xi * d1 + z));
    u = fx * x / (alpha * d2 + (1.0 - alpha) * (xi * d1 + z)) + cx;
    v = fy * y / (alpha * d2 + (1.0 - alpha) * (xi * d1 + z)) + cy;
  }
}

}  // namespace
