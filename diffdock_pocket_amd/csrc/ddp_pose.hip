// ddp_pose.hip - the pose update between two score-model calls (include/ddp_hip.h, ddp_pose_update): one launch for
//   modify_conformer(pos, tr_update, rot_update, torsion_updates)          reference utils/diffusion_utils.py:37-60
// = rigid move about the centre of mass (axis-angle -> matrix, utils/geometry.py:72-86), the rotatable-bond torsions applied
//   one after the other (utils/torsion.py:68-94) and the Kabsch re-alignment of the twisted conformer onto the rigid one
//   (utils/geometry.py:209-243), for all samples of the batch.  The reference does this per sample on the CPU with
//   numpy / scipy; the PyTorch-ROCm form of it is ~100 tiny launches per step and is bound by the host.
// One workgroup per sample, positions in LDS.  The optimal rotation is taken from Horn's quaternion form (largest
// eigenvector of the 4x4 matrix built from the 3x3 covariance, cyclic Jacobi in fp64 by one thread): it IS the Kabsch
// rotation including its reflection fix (always a proper rotation), without the SVD.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_horn.h"

#define DDP_POSE_THREADS 128

// block-wide sum of three floats (all threads get the result); red: LDS scratch of 3 * DDP_POSE_THREADS floats
__device__ __forceinline__ void block_sum3(float& x, float& y, float& z, float* red, int tid) {
  red[tid] = x; red[DDP_POSE_THREADS + tid] = y; red[2 * DDP_POSE_THREADS + tid] = z;
  __syncthreads();
  for (int s = DDP_POSE_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red[DDP_POSE_THREADS + tid] += red[DDP_POSE_THREADS + tid + s];
      red[2 * DDP_POSE_THREADS + tid] += red[2 * DDP_POSE_THREADS + tid + s];
    }
    __syncthreads();
  }
  x = red[0]; y = red[DDP_POSE_THREADS]; z = red[2 * DDP_POSE_THREADS];
  __syncthreads();
}

__global__ __launch_bounds__(DDP_POSE_THREADS) void ddp_pose_update_kernel(const float* __restrict__ pos_in, int n_atoms,
                                                                           const float* __restrict__ tr, const float* __restrict__ rot,
                                                                           const float* __restrict__ tor, int n_tor,
                                                                           const int32_t* __restrict__ bonds,
                                                                           const uint8_t* __restrict__ mask_rotate,
                                                                           float* __restrict__ pos_out) {
  extern __shared__ float lds[];
  float* f = lds;                       // [n][3] twisted conformer
  float* rg = lds + 3 * n_atoms;        // [n][3] rigid conformer
  float* red = rg + 3 * n_atoms;        // 3 * DDP_POSE_THREADS
  __shared__ float M[12];               // a 3x3 matrix (+ a translation) published by thread 0
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ pin = pos_in + (size_t)b * n_atoms * 3;
  const float inv_n = 1.0f / (float)n_atoms;

  // rigid move about the centre: (pos - c) R^T + tr + c
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int i = tid; i < n_atoms; i += DDP_POSE_THREADS) {
    const float x = pin[3 * i], y = pin[3 * i + 1], z = pin[3 * i + 2];
    f[3 * i] = x; f[3 * i + 1] = y; f[3 * i + 2] = z;
    sx += x; sy += y; sz += z;
  }
  block_sum3(sx, sy, sz, red, tid);
  const float cx = sx * inv_n, cy = sy * inv_n, cz = sz * inv_n;
  if (tid == 0) rotvec_to_matrix(rot[3 * b], rot[3 * b + 1], rot[3 * b + 2], M);
  __syncthreads();
  {
    const float tx = tr[3 * b] + cx, ty = tr[3 * b + 1] + cy, tz = tr[3 * b + 2] + cz;
    for (int i = tid; i < n_atoms; i += DDP_POSE_THREADS) {
      const float x = f[3 * i] - cx, y = f[3 * i + 1] - cy, z = f[3 * i + 2] - cz;
      const float ox = M[0] * x + M[1] * y + M[2] * z + tx, oy = M[3] * x + M[4] * y + M[5] * z + ty,
                  oz = M[6] * x + M[7] * y + M[8] * z + tz;
      f[3 * i] = ox; f[3 * i + 1] = oy; f[3 * i + 2] = oz;
      rg[3 * i] = ox; rg[3 * i + 1] = oy; rg[3 * i + 2] = oz;
    }
  }
  __syncthreads();
  if (tor == nullptr || n_tor == 0) {
    for (int i = tid; i < 3 * n_atoms; i += DDP_POSE_THREADS) pos_out[(size_t)b * n_atoms * 3 + i] = rg[i];
    return;
  }

  // torsions, in bond order: atoms of mask_rotate[j] turn about the axis pos[u] - pos[v] through pos[v]
  for (int j = 0; j < n_tor; ++j) {
    const int u = bonds[2 * j], v = bonds[2 * j + 1];
    const float pvx = f[3 * v], pvy = f[3 * v + 1], pvz = f[3 * v + 2];
    if (tid == 0) {
      const float ax = f[3 * u] - pvx, ay = f[3 * u + 1] - pvy, az = f[3 * u + 2] - pvz;
      const float k = tor[(size_t)b * n_tor + j] / sqrtf(ax * ax + ay * ay + az * az);
      rotvec_to_matrix(ax * k, ay * k, az * k, M);
    }
    __syncthreads();
    const uint8_t* __restrict__ mk = mask_rotate + (size_t)j * n_atoms;
    for (int i = tid; i < n_atoms; i += DDP_POSE_THREADS)
      if (mk[i]) {
        const float x = f[3 * i] - pvx, y = f[3 * i + 1] - pvy, z = f[3 * i + 2] - pvz;
        f[3 * i] = M[0] * x + M[1] * y + M[2] * z + pvx;
        f[3 * i + 1] = M[3] * x + M[4] * y + M[5] * z + pvy;
        f[3 * i + 2] = M[6] * x + M[7] * y + M[8] * z + pvz;
      }
    __syncthreads();
  }

  // Kabsch alignment of f (A) onto rg (B): centroids, covariance S[x][y] = sum (a - ca)_x (b - cb)_y
  float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
  for (int i = tid; i < n_atoms; i += DDP_POSE_THREADS) {
    ax += f[3 * i]; ay += f[3 * i + 1]; az += f[3 * i + 2];
    bx += rg[3 * i]; by += rg[3 * i + 1]; bz += rg[3 * i + 2];
  }
  block_sum3(ax, ay, az, red, tid);
  block_sum3(bx, by, bz, red, tid);
  const float cax = ax * inv_n, cay = ay * inv_n, caz = az * inv_n, cbx = bx * inv_n, cby = by * inv_n, cbz = bz * inv_n;
  float S0[3] = {0.f, 0.f, 0.f}, S1[3] = {0.f, 0.f, 0.f}, S2[3] = {0.f, 0.f, 0.f};
  for (int i = tid; i < n_atoms; i += DDP_POSE_THREADS) {
    const float x = f[3 * i] - cax, y = f[3 * i + 1] - cay, z = f[3 * i + 2] - caz;
    const float p = rg[3 * i] - cbx, q = rg[3 * i + 1] - cby, r = rg[3 * i + 2] - cbz;
    S0[0] += x * p; S0[1] += x * q; S0[2] += x * r;
    S1[0] += y * p; S1[1] += y * q; S1[2] += y * r;
    S2[0] += z * p; S2[1] += z * q; S2[2] += z * r;
  }
  block_sum3(S0[0], S0[1], S0[2], red, tid);
  block_sum3(S1[0], S1[1], S1[2], red, tid);
  block_sum3(S2[0], S2[1], S2[2], red, tid);
  if (tid == 0) {
    const float S[9] = {S0[0], S0[1], S0[2], S1[0], S1[1], S1[2], S2[0], S2[1], S2[2]}, ca[3] = {cax, cay, caz}, cb[3] = {cbx, cby, cbz};
    float R[9], t[3];
    horn_rigid(S, ca, cb, R, t);
    for (int k = 0; k < 9; ++k) M[k] = R[k];
    for (int k = 0; k < 3; ++k) M[9 + k] = t[k];
  }
  __syncthreads();
  float* __restrict__ po = pos_out + (size_t)b * n_atoms * 3;
  for (int i = tid; i < n_atoms; i += DDP_POSE_THREADS) {
    const float x = f[3 * i], y = f[3 * i + 1], z = f[3 * i + 2];
    po[3 * i] = M[0] * x + M[1] * y + M[2] * z + M[9];
    po[3 * i + 1] = M[3] * x + M[4] * y + M[5] * z + M[10];
    po[3 * i + 2] = M[6] * x + M[7] * y + M[8] * z + M[11];
  }
}

extern "C" int ddp_pose_update(const float* pos_in, int n_samples, int n_atoms, const float* tr, const float* rot,
                               const float* tor, int n_tor, const int32_t* bonds, const uint8_t* mask_rotate, float* pos_out,
                               void* stream) {
  if (n_samples <= 0 || n_atoms <= 0) return 0;
  if (!pos_in || !tr || !rot || !pos_out) return ddp_fail(DDP_EINVAL, "ddp_pose_update: null argument");
  if (n_tor < 0 || (n_tor > 0 && tor && (!bonds || !mask_rotate))) return ddp_fail(DDP_EINVAL, "ddp_pose_update: torsion arguments");
  const size_t lds = (size_t)(6 * n_atoms + 3 * DDP_POSE_THREADS) * sizeof(float);
  if (lds > 60 * 1024) return ddp_fail(DDP_ELIMIT, "ddp_pose_update: more than 2400 atoms per sample");
  hipLaunchKernelGGL(ddp_pose_update_kernel, dim3(n_samples), dim3(DDP_POSE_THREADS), lds, (hipStream_t)stream, pos_in, n_atoms,
                     tr, rot, tor, n_tor, bonds, mask_rotate, pos_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_pose_update launch");
  return 0;
}

// ---- side-chain torsion update (modify_sidechains, utils/diffusion_utils.py:63-70 / utils/torsion.py:251-278): for every
// sample the flexible-residue bonds are applied one after the other; bond j turns the atoms subcomponents[map[j][0] ..
// map[j][1]) by angles[s][j] about pos[u_j] - pos[v_j] through pos[v_j].  One workgroup per sample; the PyTorch form is
// ~9 launches per bond.
__global__ __launch_bounds__(64) void ddp_sidechain_update_kernel(const float* __restrict__ pos_in, int n_atoms,
                                                                  const float* __restrict__ angles, int n_bonds,
                                                                  const int32_t* __restrict__ edge_idx,
                                                                  const int32_t* __restrict__ subcomponents,
                                                                  const int32_t* __restrict__ mapping,
                                                                  float* __restrict__ pos_out) {
  __shared__ float M[12];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ pin = pos_in + (size_t)b * n_atoms * 3;
  float* po = pos_out + (size_t)b * n_atoms * 3;
  if (pin != po)
    for (int i = tid; i < 3 * n_atoms; i += 64) po[i] = pin[i];
  __syncthreads();
  for (int j = 0; j < n_bonds; ++j) {
    const int u = edge_idx[2 * j], v = edge_idx[2 * j + 1];
    if (tid == 0) {
      const float pvx = po[3 * v], pvy = po[3 * v + 1], pvz = po[3 * v + 2];
      const float ax = po[3 * u] - pvx, ay = po[3 * u + 1] - pvy, az = po[3 * u + 2] - pvz;
      const float k = angles[(size_t)b * n_bonds + j] / sqrtf(ax * ax + ay * ay + az * az);
      rotvec_to_matrix(ax * k, ay * k, az * k, M);
      M[9] = pvx; M[10] = pvy; M[11] = pvz;
    }
    __syncthreads();
    const int m0 = mapping[2 * j], m1 = mapping[2 * j + 1];
    for (int i = m0 + tid; i < m1; i += 64) {
      const int a = subcomponents[i];
      const float x = po[3 * a] - M[9], y = po[3 * a + 1] - M[10], z = po[3 * a + 2] - M[11];
      po[3 * a] = M[0] * x + M[1] * y + M[2] * z + M[9];
      po[3 * a + 1] = M[3] * x + M[4] * y + M[5] * z + M[10];
      po[3 * a + 2] = M[6] * x + M[7] * y + M[8] * z + M[11];
    }
    __syncthreads();   // block-wide visibility of the moved atoms before the next bond reads its axis
  }
}

extern "C" int ddp_sidechain_update(const float* pos_in, int n_samples, int n_atoms, const float* angles, int n_bonds,
                                    const int32_t* edge_idx, const int32_t* subcomponents, const int32_t* mapping, float* pos_out,
                                    void* stream) {
  if (n_samples <= 0 || n_atoms <= 0) return 0;
  if (!pos_in || !pos_out || (n_bonds > 0 && (!angles || !edge_idx || !subcomponents || !mapping)))
    return ddp_fail(DDP_EINVAL, "ddp_sidechain_update: null argument");
  hipLaunchKernelGGL(ddp_sidechain_update_kernel, dim3(n_samples), dim3(64), 0, (hipStream_t)stream, pos_in, n_atoms, angles,
                     n_bonds, edge_idx, subcomponents, mapping, pos_out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_sidechain_update launch");
  return 0;
}

// ---- scores -> pose updates: the reverse SDE / ODE step of utils/sampling.py:146-193 for the four components at once,
//   out[k][i] = a[k] * score[k][i] + b[k] * z[k][i],   coef = [a_tr b_tr a_rot b_rot a_tor b_tor a_sc b_sc] in DEVICE memory
// (a = g^2 dt (lambda + temp psi / 2), b = g sqrt(dt (1 + psi)) with low-temperature sampling; the host writes them per step
// together with the noise, so a captured step needs no kernel arguments that change).  Products and sum are rounded
// separately, as the PyTorch expression `a * score + b * z` does.
struct SdeLaunch {
  ddp_sde_args_t a;
};
__global__ __launch_bounds__(256) void ddp_sde_update_kernel(const float* __restrict__ coef, const SdeLaunch L) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i < L.a.n[k]) {
      const float p = coef[2 * k] * L.a.score[k][i];
      const float q = L.a.z[k] ? coef[2 * k + 1] * L.a.z[k][i] : 0.f;
      L.a.out[k][i] = L.a.z[k] ? p + q : p;
    }
  }
}

extern "C" int ddp_sde_update(const float* coef, const ddp_sde_args_t* args, void* stream) {
  if (!coef || !args) return ddp_fail(DDP_EINVAL, "ddp_sde_update: null argument");
  int nmax = 0;
  for (int k = 0; k < 4; ++k) {
    if (args->n[k] < 0 || (args->n[k] > 0 && (!args->score[k] || !args->out[k]))) return ddp_fail(DDP_EINVAL, "ddp_sde_update: component");
    if (args->n[k] > nmax) nmax = args->n[k];
  }
  if (nmax == 0) return 0;
  SdeLaunch L;
  L.a = *args;
  hipLaunchKernelGGL(ddp_sde_update_kernel, dim3((nmax + 255) / 256), dim3(256), 0, (hipStream_t)stream, coef, L);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_sde_update launch");
  return 0;
}
