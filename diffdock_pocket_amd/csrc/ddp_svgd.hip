// ddp_svgd.hip - the Stein variational (SVGD) particle-interaction term of the reverse-diffusion step (include/ddp_hip.h,
// ddp_svgd_*; reference utils/sampling.py:197-242, utils/torsion.py:96-160, utils/geometry.py:100-206,246-281): the one place where the
// N samples of a complex interact.  The reference does it on the host with a Python double loop of N (N - 1) / 2 3x3 SVDs per step;
// here it is three launches between ddp_sde_update and ddp_pose_update, captured with the step:
//   ddp_svgd_tau    one thread per (sample, rotatable bond): the signed dihedral angle
//   ddp_svgd_pairs  one workgroup per pair i <= j: centroids, 3x3 covariance, Kabsch rotation (Horn's quaternion, ddp_horn.h) in the
//                   reference's axis-angle convention, wrapped torsion differences, the distance D - written for (i, j) and (j, i)
//   ddp_svgd_rows   one workgroup per sample i: lower median of row i of D by rank selection, the bandwidth h_i, the kernel row
//                   k[i][:] and the attractive + repulsive sums in ascending j, added into the step's update buffers
// Arithmetic is fp64 throughout (a few thousand operations per pair at N = 40), stored as fp32 except tau and D.  No atomics: every output
// element has one writer and every sum a fixed order, so a replayed step repeats a launched one bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_horn.h"

#define DDP_SVGD_PAIR_THREADS 64
#define DDP_SVGD_ROW_THREADS 256
#define DDP_SVGD_PI 3.141592653589793238462643383279502884

struct SvgdLaunch {
  ddp_svgd_args_t a;
};

// ---- tau[s][t]: dihedral (c, a, b, d) of sample s, utils/torsion.py:120-135 with the cross product over xyz
__global__ __launch_bounds__(64) void ddp_svgd_tau_kernel(const SvgdLaunch L) {
  const ddp_svgd_args_t& A = L.a;
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= A.n * A.n_tor) return;
  const int s = idx / A.n_tor, t = idx % A.n_tor;
  const float* __restrict__ p = A.pos + (size_t)s * A.n_lig * 3;
  double P[4][3];
  for (int k = 0; k < 4; ++k) {
    const int at = A.dihedrals[4 * t + k];
    for (int x = 0; x < 3; ++x) P[k][x] = (double)p[3 * at + x];
  }
  // c = P[0], a = P[1], b = P[2], d = P[3]
  double ab[3], ca[3], da[3];
  double abab = 0.0, caab = 0.0, daab = 0.0;
  for (int x = 0; x < 3; ++x) {
    ab[x] = P[2][x] - P[1][x];
    ca[x] = P[0][x] - P[1][x];
    da[x] = P[3][x] - P[1][x];
    abab += ab[x] * ab[x];
    caab += ca[x] * ab[x];
    daab += da[x] * ab[x];
  }
  // u = d - proj_ab(d), v = c - proj_ab(c): the parts of d - a and c - a normal to the axis
  double u[3], v[3], uv = 0.0, uu = 0.0, vv = 0.0;
  for (int x = 0; x < 3; ++x) {
    u[x] = da[x] - daab / abab * ab[x];
    v[x] = ca[x] - caab / abab * ab[x];
    uv += u[x] * v[x];
    uu += u[x] * u[x];
    vv += v[x] * v[x];
  }
  double c = uv / (sqrt(uu) * sqrt(vv));
  c = fmin(fmax(c, -1.0 + 1e-5), 1.0 - 1e-5);
  const double triple = (u[1] * v[2] - u[2] * v[1]) * ab[0] + (u[2] * v[0] - u[0] * v[2]) * ab[1] + (u[0] * v[1] - u[1] * v[0]) * ab[2];
  const double sign = triple > 0.0 ? 1.0 : (triple < 0.0 ? -1.0 : 0.0);
  A.tau[idx] = acos(c) * sign;
}

// block-wide sum of NV doubles per thread (all threads get the results); red: NV * DDP_SVGD_PAIR_THREADS doubles of LDS
template <int NV>
__device__ __forceinline__ void pair_sum(double* v, double* red, int tid) {
  for (int k = 0; k < NV; ++k) red[k * DDP_SVGD_PAIR_THREADS + tid] = v[k];
  __syncthreads();
  for (int s = DDP_SVGD_PAIR_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < NV; ++k) red[k * DDP_SVGD_PAIR_THREADS + tid] += red[k * DDP_SVGD_PAIR_THREADS + tid + s];
    __syncthreads();
  }
  for (int k = 0; k < NV; ++k) v[k] = red[k * DDP_SVGD_PAIR_THREADS];
  __syncthreads();
}

__device__ __forceinline__ double wrap_diff(double ti, double tj) {
  return fmod(ti - tj + 3.0 * DDP_SVGD_PI, 2.0 * DDP_SVGD_PI) - DDP_SVGD_PI;
}

// ---- pair (i, j), i <= j: blockIdx.x = j, blockIdx.y = i (blocks below the diagonal have nothing to do)
__global__ __launch_bounds__(DDP_SVGD_PAIR_THREADS) void ddp_svgd_pairs_kernel(const SvgdLaunch L) {
  const ddp_svgd_args_t& A = L.a;
  __shared__ double red[9 * DDP_SVGD_PAIR_THREADS];
  __shared__ double rig[8];     // tr_diff, rot_diff, |tr|^2, |rot|^2 published by thread 0
  const int i = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  if (i > j) return;
  const int N = A.n, n = A.n_lig, T = A.n_tor;
  const size_t ij = (size_t)i * N + j, ji = (size_t)j * N + i;
  if (i < j) {
    const float* __restrict__ pa = A.pos + (size_t)i * n * 3;
    const float* __restrict__ pb = A.pos + (size_t)j * n * 3;
    double c[6] = {0, 0, 0, 0, 0, 0};
    for (int k = tid; k < n; k += DDP_SVGD_PAIR_THREADS)
      for (int x = 0; x < 3; ++x) {
        c[x] += (double)pa[3 * k + x];
        c[3 + x] += (double)pb[3 * k + x];
      }
    pair_sum<6>(c, red, tid);
    for (int x = 0; x < 6; ++x) c[x] /= (double)n;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = tid; k < n; k += DDP_SVGD_PAIR_THREADS) {
      double a[3], b[3];
      for (int x = 0; x < 3; ++x) {
        a[x] = (double)pa[3 * k + x] - c[x];
        b[x] = (double)pb[3 * k + x] - c[3 + x];
      }
      for (int x = 0; x < 3; ++x)
        for (int y = 0; y < 3; ++y) H[3 * x + y] += a[x] * b[y];
    }
    pair_sum<9>(H, red, tid);
    if (tid == 0) {
      const double S[3][3] = {{H[0], H[1], H[2]}, {H[3], H[4], H[5]}, {H[6], H[7], H[8]}};
      double q[4];
      horn_quaternion(S, q);
      // matrix_to_quaternion (utils/geometry.py:100-159) returns the candidate whose own component is largest in magnitude, that
      // component positive (q_abs[k] = 2 |q_k|; first maximum as argmax), and does not standardise the sign of w
      int best = 0;
      for (int k = 1; k < 4; ++k)
        if (fabs(q[k]) > fabs(q[best])) best = k;
      const double sg = q[best] < 0.0 ? -1.0 : 1.0;
      const double w = sg * q[0], x = sg * q[1], y = sg * q[2], z = sg * q[3];
      // quaternion_to_axis_angle (:162-190): angle = 2 atan2(|xyz|, w) in [0, 2 pi): the vector can be longer than pi
      const double nrm = sqrt(x * x + y * y + z * z);
      const double half = atan2(nrm, w), ang = 2.0 * half;
      const double sha = fabs(ang) < 1e-6 ? 0.5 - ang * ang / 48.0 : sin(half) / ang;
      rig[0] = c[3] - c[0]; rig[1] = c[4] - c[1]; rig[2] = c[5] - c[2];
      rig[3] = x / sha; rig[4] = y / sha; rig[5] = z / sha;
      rig[6] = rig[0] * rig[0] + rig[1] * rig[1] + rig[2] * rig[2];
      rig[7] = rig[3] * rig[3] + rig[4] * rig[4] + rig[5] * rig[5];
    }
  } else if (tid == 0) {
    for (int k = 0; k < 8; ++k) rig[k] = 0.0;
  }
  __syncthreads();
  if (tid < 6) {
    const float v = (float)rig[tid];
    float* dst = tid < 3 ? A.tr_diff : A.rot_diff;
    dst[3 * ij + tid % 3] = v;
    if (i < j) dst[3 * ji + tid % 3] = -v;     // the lower triangle is the negated mirror of the upper one
  }
  // torsion differences: (i, j) and (j, i) each by the wrap formula (they are not mirrors of each other at +-pi)
  double tm[2] = {0.0, 0.0};
  for (int t = tid; t < T; t += DDP_SVGD_PAIR_THREADS) {
    const double ti = A.tau[(size_t)i * T + t], tj = A.tau[(size_t)j * T + t];
    const double dij = wrap_diff(ti, tj), dji = wrap_diff(tj, ti);
    A.tor_diff[ij * T + t] = (float)dij;
    if (i < j) A.tor_diff[ji * T + t] = (float)dji;
    tm[0] += dij * dij;
    tm[1] += dji * dji;
  }
  pair_sum<2>(tm, red, tid);
  if (tid == 0) {
    const double rigid = rig[6] + (double)A.w_rot * rig[7];
    A.dist[ij] = rigid + (double)A.w_tor * tm[0];
    if (i < j) A.dist[ji] = rigid + (double)A.w_tor * tm[1];
  }
}

// ---- row i: h_i from the lower median of D[i][:], k[i][:], the sums over j in ascending order, the update
__global__ __launch_bounds__(DDP_SVGD_ROW_THREADS) void ddp_svgd_rows_kernel(const SvgdLaunch L) {
  const ddp_svgd_args_t& A = L.a;
  extern __shared__ double row[];       // [N] D[i][:], overwritten by k[i][:]; [N]: the row's median
  const int i = blockIdx.x, tid = threadIdx.x, N = A.n, T = A.n_tor;
  for (int j = tid; j < N; j += DDP_SVGD_ROW_THREADS) row[j] = A.dist[(size_t)i * N + j];
  __syncthreads();
  // torch.median: the element of rank (N - 1) / 2 in ascending order (the lower middle value of an even N); ranks are made
  // unique by the index, so exactly one thread publishes
  for (int j = tid; j < N; j += DDP_SVGD_ROW_THREADS) {
    const double v = row[j];
    int rank = 0;
    for (int m = 0; m < N; ++m) rank += (row[m] < v || (row[m] == v && m < j)) ? 1 : 0;
    if (rank == (N - 1) / 2) row[N] = v;
  }
  __syncthreads();
  const double lnN = log((double)N);
  const double h = (double)A.w_rep * row[N] / (lnN > 1.0 ? lnN : 1.0);
  __syncthreads();
  for (int j = tid; j < N; j += DDP_SVGD_ROW_THREADS) row[j] = exp(-row[j] / h);
  __syncthreads();
  // component c of the concatenated (tr[3], rot[3], tor[T]) update of sample i
  for (int c = tid; c < 6 + T; c += DDP_SVGD_ROW_THREADS) {
    const int X = c < 3 ? 0 : (c < 6 ? 1 : 2), cc = c < 3 ? c : (c < 6 ? c - 3 : c - 6), ld = X == 2 ? T : 3;
    const float* __restrict__ score = A.score[X];
    const float* __restrict__ diff = (X == 0 ? A.tr_diff : (X == 1 ? A.rot_diff : A.tor_diff)) + (size_t)i * N * ld;
    const double wX = X == 0 ? 1.0 : (X == 1 ? (double)A.w_rot : (double)A.w_tor);
    double att = 0.0, rep = 0.0;
    for (int j = 0; j < N; ++j) {
      att += row[j] * (double)score[(size_t)j * ld + cc];
      rep += 2.0 / h * wX * (double)diff[(size_t)j * ld + cc] * row[j];
    }
    const double total = (double)A.gdt[X] * (att + rep) / (double)N;
    float* out = A.upd[X] + (size_t)i * ld + cc;
    *out = (float)((A.svgd_only ? 0.0 : (double)*out) + (double)A.weight * total);
  }
}

static int svgd_check(const ddp_svgd_args_t* a, const char* who) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_svgd: null argument");
  if (a->n < 3) return ddp_fail(DDP_EINVAL, "ddp_svgd: fewer than 3 samples (the median of a two-sample row is its zero diagonal)");
  if (a->n_lig < 4 || a->n_tor < 0) return ddp_fail(DDP_EINVAL, "ddp_svgd: n_lig < 4 or n_tor < 0");
  if (a->n > 2048) return ddp_fail(DDP_ELIMIT, "ddp_svgd: more than 2048 samples");
  if (!a->pos || !a->tr_diff || !a->rot_diff || !a->dist) return ddp_fail(DDP_EINVAL, "ddp_svgd: null pose or workspace pointer");
  if (a->n_tor > 0 && (!a->dihedrals || !a->tau || !a->tor_diff)) return ddp_fail(DDP_EINVAL, "ddp_svgd: null torsion pointer");
  (void)who;
  return 0;
}

extern "C" int ddp_svgd_tau(const ddp_svgd_args_t* args, void* stream) {
  if (const int rc = svgd_check(args, "ddp_svgd_tau")) return rc;
  if (args->n_tor == 0) return 0;
  SvgdLaunch L;
  L.a = *args;
  hipLaunchKernelGGL(ddp_svgd_tau_kernel, dim3((args->n * args->n_tor + 63) / 64), dim3(64), 0, (hipStream_t)stream, L);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_svgd_tau launch");
  return 0;
}

extern "C" int ddp_svgd_pairs(const ddp_svgd_args_t* args, void* stream) {
  if (const int rc = svgd_check(args, "ddp_svgd_pairs")) return rc;
  SvgdLaunch L;
  L.a = *args;
  hipLaunchKernelGGL(ddp_svgd_pairs_kernel, dim3(args->n, args->n), dim3(DDP_SVGD_PAIR_THREADS), 0, (hipStream_t)stream, L);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_svgd_pairs launch");
  return 0;
}

extern "C" int ddp_svgd_rows(const ddp_svgd_args_t* args, void* stream) {
  if (const int rc = svgd_check(args, "ddp_svgd_rows")) return rc;
  if (!args->gdt || !args->score[0] || !args->score[1] || !args->upd[0] || !args->upd[1] ||
      (args->n_tor > 0 && (!args->score[2] || !args->upd[2])))
    return ddp_fail(DDP_EINVAL, "ddp_svgd_rows: null score, update or coefficient pointer");
  SvgdLaunch L;
  L.a = *args;
  hipLaunchKernelGGL(ddp_svgd_rows_kernel, dim3(args->n), dim3(DDP_SVGD_ROW_THREADS), (size_t)(args->n + 1) * sizeof(double),
                     (hipStream_t)stream, L);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_svgd_rows launch");
  return 0;
}
