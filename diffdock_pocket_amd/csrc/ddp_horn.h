// ddp_horn.h - the rotations of the pose map, shared by the pose update (ddp_pose.hip), the fused minimiser (ddp_minimize.hip) and the
// SVGD pair pass (ddp_svgd.hip).  Horn's quaternion form of the optimal rotation between two point sets: the unit quaternion of the
// Kabsch rotation (reflection fix included: always a proper rotation) is the eigenvector of the largest eigenvalue of a symmetric 4x4
// matrix built from the 3x3 covariance.  And the axis-angle vector -> matrix step of the rigid move and the torsions.
#ifndef DDP_HORN_H
#define DDP_HORN_H
#include <hip/hip_runtime.h>

__device__ __forceinline__ void rotvec_to_matrix(float vx, float vy, float vz, float* R) {
  // Rodrigues; small-angle series below 1e-6 as in sampler.rotvec_to_matrix / scipy
  const float ang = sqrtf(vx * vx + vy * vy + vz * vz);
  float a, b;
  if (ang < 1e-6f) {
    a = 1.0f - ang * ang / 6.0f;
    b = 0.5f - ang * ang / 24.0f;
  } else {
    a = sinf(ang) / ang;
    b = (1.0f - cosf(ang)) / (ang * ang);
  }
  // K = [[0,-z,y],[z,0,-x],[-y,x,0]];  R = I + a K + b K^2
  const float xx = vx * vx, yy = vy * vy, zz = vz * vz, xy = vx * vy, xz = vx * vz, yz = vy * vz;
  R[0] = 1.f - b * (yy + zz); R[1] = -a * vz + b * xy;     R[2] = a * vy + b * xz;
  R[3] = a * vz + b * xy;     R[4] = 1.f - b * (xx + zz);  R[5] = -a * vx + b * yz;
  R[6] = -a * vy + b * xz;    R[7] = a * vx + b * yz;      R[8] = 1.f - b * (xx + yy);
}

// largest-eigenvalue eigenvector of the symmetric 4x4 matrix A (cyclic Jacobi, fp64)
static __device__ void max_eigvec4(double A[4][4], double q[4]) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < 4; ++p)
      for (int r = 0; r < 4; ++r) (p == r ? diag : off) += A[p][r] * A[p][r];
    if (off <= 1e-30 * diag || off == 0.0) break;
    for (int p = 0; p < 3; ++p)
      for (int r = p + 1; r < 4; ++r) {
        if (fabs(A[p][r]) < 1e-300) continue;
        const double theta = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {   // A <- A J
          const double akp = A[k][p], akr = A[k][r];
          A[k][p] = c * akp - s * akr;
          A[k][r] = s * akp + c * akr;
        }
        for (int k = 0; k < 4; ++k) {   // A <- J^T A
          const double apk = A[p][k], ark = A[r][k];
          A[p][k] = c * apk - s * ark;
          A[r][k] = s * apk + c * ark;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkr = V[k][r];
          V[k][p] = c * vkp - s * vkr;
          V[k][r] = s * vkp + c * vkr;
        }
      }
  }
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > A[best][best]) best = k;
  for (int k = 0; k < 4; ++k) q[k] = V[k][best];
}

// S[x][y] = sum_k (a_k - ca)_x (b_k - cb)_y  ->  unit quaternion (w, x, y, z) of the rotation R with R (a - ca) ~ (b - cb)
static __device__ void horn_quaternion(const double S[3][3], double q[4]) {
  const double Sxx = S[0][0], Sxy = S[0][1], Sxz = S[0][2], Syx = S[1][0], Syy = S[1][1], Syz = S[1][2], Szx = S[2][0], Szy = S[2][1],
               Szz = S[2][2];
  double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  max_eigvec4(N, q);
  const double nq = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] *= nq;
}

// fp32 covariance S (row-major, as above) and centroids ca, cb  ->  the fp32 rigid map b ~ R a + t: the quaternion in fp64, the
// matrix rounded to fp32, t = cb - R ca in fp32
__device__ __forceinline__ void horn_rigid(const float* S, const float* ca, const float* cb, float* R, float* t) {
  const double S3[3][3] = {{S[0], S[1], S[2]}, {S[3], S[4], S[5]}, {S[6], S[7], S[8]}};
  double q[4];
  horn_quaternion(S3, q);
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = (float)(1 - 2 * (y * y + z * z)); R[1] = (float)(2 * (x * y - z * w)); R[2] = (float)(2 * (x * z + y * w));
  R[3] = (float)(2 * (x * y + z * w)); R[4] = (float)(1 - 2 * (x * x + z * z)); R[5] = (float)(2 * (y * z - x * w));
  R[6] = (float)(2 * (x * z - y * w)); R[7] = (float)(2 * (y * z + x * w)); R[8] = (float)(1 - 2 * (x * x + y * y));
  for (int k = 0; k < 3; ++k) t[k] = cb[k] - (R[3 * k] * ca[0] + R[3 * k + 1] * ca[1] + R[3 * k + 2] * ca[2]);
}

#endif
