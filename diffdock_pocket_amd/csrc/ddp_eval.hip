// ddp_eval.hip - evaluation of sampled poses against a reference pose (include/ddp_hip.h, ddp_pose_rmsd / ddp_pose_contacts):
//   symmetry-corrected RMSD (spyrmsd symmrmsd as called by utils/utils.py:116-130: no centring, no alignment, minimum over the
//   graph automorphisms), plain and side-chain RMSD (evaluate_files.py:150-154,237), centroid distance, minimum ligand-receptor /
//   ligand-ligand distances (evaluate_files.py:251-256) and the receptor-ligand steric-clash count (datasets/steric_clash.py:99-136).
// One 256-thread workgroup per sample, coordinates staged in LDS.  Every reduction is a fixed tree (wave shuffles, then the 4 waves
// through LDS) of an order-independent operation (integer sum, min, (value, index) min) or a fixed-order loop: no atomics, the same
// bits on every launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"

#define DDP_EVAL_THREADS 256
#define DDP_EVAL_WAVES (DDP_EVAL_THREADS / 64)

// (value, index) minimum with ties to the lower index; an index < 0 marks "none" and loses to every valid entry
__device__ __forceinline__ bool better(double v, int p, double w, int q) {
  if (q < 0) return p >= 0;
  if (p < 0) return false;
  return v < w || (v == w && p < q);
}

// ---- rmsd[s] = min_p sqrt(sum_i |pred_s[sel_i] - ref[perms[i, p]]|^2 / n)
// LDS: the sample's n selected coordinates and the n_ref reference rows.  Lane t walks p = t, t + 256, ... (perms is atom-major,
// so the 64 lanes of a wave read 64 consecutive ints per atom); each sum runs over i in increasing order, squares accumulated in fp64.
__global__ __launch_bounds__(DDP_EVAL_THREADS) void ddp_pose_rmsd_kernel(const float* __restrict__ pred, int pred_stride,
                                                                        const int32_t* __restrict__ sel, int n,
                                                                        const float* __restrict__ ref, int n_ref,
                                                                        const int32_t* __restrict__ perms, int P,
                                                                        float* __restrict__ rmsd, int32_t* __restrict__ best) {
  extern __shared__ float lds[];
  float* x = lds;              // [n][3] selected coordinates of sample s
  float* r = lds + 3 * n;      // [n_ref][3]
  __shared__ double wv[DDP_EVAL_WAVES];
  __shared__ int wp[DDP_EVAL_WAVES];
  __shared__ int bad_sel;
  const int s = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ ps = pred + (size_t)s * pred_stride;
  if (tid == 0) bad_sel = 0;
  __syncthreads();
  for (int i = tid; i < n; i += DDP_EVAL_THREADS) {
    const int row = sel ? sel[i] : i;
    if (row < 0 || 3 * row + 2 >= pred_stride) {       // a selected row outside the sample's row: no read, the sample gets NaN
      bad_sel = 1;
      continue;
    }
    x[3 * i] = ps[3 * row]; x[3 * i + 1] = ps[3 * row + 1]; x[3 * i + 2] = ps[3 * row + 2];
  }
  for (int i = tid; i < 3 * n_ref; i += DDP_EVAL_THREADS) r[i] = ref[i];
  __syncthreads();
  if (bad_sel) {
    if (tid == 0) { rmsd[s] = __builtin_nanf(""); best[s] = -1; }
    return;
  }
  double bv = 0.0;
  int bp = -1;
  for (int p = tid; p < P; p += DDP_EVAL_THREADS) {
    double acc = 0.0;
    bool ok = true;
    for (int i = 0; i < n; ++i) {
      const int q = perms[(size_t)i * P + p];
      if (q < 0 || q >= n_ref) { ok = false; break; }   // an entry outside ref: this permutation is not considered
      const float dx = x[3 * i] - r[3 * q], dy = x[3 * i + 1] - r[3 * q + 1], dz = x[3 * i + 2] - r[3 * q + 2];
      acc += (double)dx * dx + (double)dy * dy + (double)dz * dz;
    }
    if (ok && better(acc, p, bv, bp)) { bv = acc; bp = p; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(bv, off);
    const int op = __shfl_xor(bp, off);
    if (better(ov, op, bv, bp)) { bv = ov; bp = op; }
  }
  if ((tid & 63) == 0) { wv[tid >> 6] = bv; wp[tid >> 6] = bp; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < DDP_EVAL_WAVES; ++w)
      if (better(wv[w], wp[w], bv, bp)) { bv = wv[w]; bp = wp[w]; }
    rmsd[s] = bp >= 0 ? (float)sqrt(bv / (double)n) : __builtin_nanf("");
    best[s] = bp;
  }
}

extern "C" int ddp_pose_rmsd(const float* pred, int n_samples, int pred_stride, const int32_t* sel, int n, const float* ref, int n_ref,
                             const int32_t* perms, int n_perms, float* rmsd, int32_t* best, void* stream) {
  if (n_samples == 0) return 0;
  if (n_samples < 0 || n <= 0 || n_ref <= 0 || n_perms <= 0 || pred_stride < 3) return ddp_fail(DDP_EINVAL, "ddp_pose_rmsd: shape");
  if (!pred || !ref || !perms || !rmsd || !best) return ddp_fail(DDP_EINVAL, "ddp_pose_rmsd: null argument");
  if (!sel && 3 * n > pred_stride) return ddp_fail(DDP_EINVAL, "ddp_pose_rmsd: n rows do not fit in pred_stride");
  if (n > DDP_EVAL_MAX_ATOMS || n_ref > DDP_EVAL_MAX_ATOMS) return ddp_fail(DDP_ELIMIT, "ddp_pose_rmsd: more than DDP_EVAL_MAX_ATOMS atoms");
  const size_t lds = (size_t)3 * (n + n_ref) * sizeof(float);
  hipLaunchKernelGGL(ddp_pose_rmsd_kernel, dim3(n_samples), dim3(DDP_EVAL_THREADS), lds, (hipStream_t)stream, pred, pred_stride, sel, n,
                     ref, n_ref, perms, n_perms, rmsd, best);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_pose_rmsd launch");
  return 0;
}

// ---- contacts of sample s: out[s] = [clash count, min ligand-receptor distance, min ligand-ligand distance (i != j), centroid distance]
// The ligand (coordinates + radii) is staged in LDS; lane t walks the receptor atoms j = t, t + 256, ... against every ligand atom, then
// the ligand pairs k = t, t + 256, ... of the n x n square.  A pair clashes when r_i + r_j - 2 overlap > 0 and d^2 < (r_i + r_j -
// 2 overlap)^2 (= d < r_i + r_j - 2 overlap); a receptor atom with r_j < 0 takes part in the minimum only.  Minima are taken over
// squared distances in fp32 (the square root is monotonic); an empty set gives +inf, as the reference's np.min over inf-masked pairs.
__global__ __launch_bounds__(DDP_EVAL_THREADS) void ddp_pose_contacts_kernel(const float* __restrict__ lig, int n,
                                                                            const float* __restrict__ lig_radii,
                                                                            const float* __restrict__ rec, int m, int rec_stride,
                                                                            const float* __restrict__ rec_radii, float overlap,
                                                                            const float* __restrict__ ref_centroid,
                                                                            float* __restrict__ out) {
  extern __shared__ float lds[];
  float* x = lds;              // [n][3]
  float* rad = lds + 3 * n;    // [n]
  __shared__ int wc[DDP_EVAL_WAVES];
  __shared__ float wx[DDP_EVAL_WAVES], wl[DDP_EVAL_WAVES];
  const int s = blockIdx.x, tid = threadIdx.x;
  const float* __restrict__ ls = lig + (size_t)s * n * 3;
  const float* __restrict__ rs = rec + (size_t)s * rec_stride;
  for (int i = tid; i < 3 * n; i += DDP_EVAL_THREADS) x[i] = ls[i];
  for (int i = tid; i < n; i += DDP_EVAL_THREADS) rad[i] = lig_radii[i];
  __syncthreads();
  const float two_ov = 2.0f * overlap;
  int clashes = 0;
  float dmin = INFINITY, smin = INFINITY;
  for (int j = tid; j < m; j += DDP_EVAL_THREADS) {
    const float px = rs[3 * j], py = rs[3 * j + 1], pz = rs[3 * j + 2], rj = rec_radii[j];
    for (int i = 0; i < n; ++i) {
      const float dx = x[3 * i] - px, dy = x[3 * i + 1] - py, dz = x[3 * i + 2] - pz;
      const float d2 = dx * dx + dy * dy + dz * dz;
      dmin = fminf(dmin, d2);
      const float t = rad[i] + rj - two_ov;
      clashes += (rj >= 0.f && t > 0.f && d2 < t * t) ? 1 : 0;
    }
  }
  for (int k = tid; k < n * n; k += DDP_EVAL_THREADS) {
    const int i = k / n, j = k - i * n;
    if (i == j) continue;
    const float dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
    smin = fminf(smin, dx * dx + dy * dy + dz * dz);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    clashes += __shfl_xor(clashes, off);
    dmin = fminf(dmin, __shfl_xor(dmin, off));
    smin = fminf(smin, __shfl_xor(smin, off));
  }
  if ((tid & 63) == 0) { wc[tid >> 6] = clashes; wx[tid >> 6] = dmin; wl[tid >> 6] = smin; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < DDP_EVAL_WAVES; ++w) { clashes += wc[w]; dmin = fminf(dmin, wx[w]); smin = fminf(smin, wl[w]); }
    double cx = 0.0, cy = 0.0, cz = 0.0;      // centroid: fixed-order fp64 sum
    for (int i = 0; i < n; ++i) { cx += x[3 * i]; cy += x[3 * i + 1]; cz += x[3 * i + 2]; }
    cx = cx / n - ref_centroid[0]; cy = cy / n - ref_centroid[1]; cz = cz / n - ref_centroid[2];
    float* o = out + 4 * (size_t)s;
    o[0] = (float)clashes;
    o[1] = sqrtf(dmin);
    o[2] = sqrtf(smin);
    o[3] = (float)sqrt(cx * cx + cy * cy + cz * cz);
  }
}

extern "C" int ddp_pose_contacts(const float* lig, int n_samples, int n, const float* lig_radii, const float* rec, int m, int rec_stride,
                                 const float* rec_radii, float overlap, const float* ref_centroid, float* out, void* stream) {
  if (n_samples == 0) return 0;
  if (n_samples < 0 || n <= 0 || m < 0 || (rec_stride != 0 && rec_stride < 3 * m)) return ddp_fail(DDP_EINVAL, "ddp_pose_contacts: shape");
  if (!lig || !lig_radii || !ref_centroid || !out || (m > 0 && (!rec || !rec_radii)))
    return ddp_fail(DDP_EINVAL, "ddp_pose_contacts: null argument");
  if (n > DDP_EVAL_MAX_ATOMS) return ddp_fail(DDP_ELIMIT, "ddp_pose_contacts: more than DDP_EVAL_MAX_ATOMS ligand atoms");
  const size_t lds = (size_t)4 * n * sizeof(float);
  hipLaunchKernelGGL(ddp_pose_contacts_kernel, dim3(n_samples), dim3(DDP_EVAL_THREADS), lds, (hipStream_t)stream, lig, n, lig_radii,
                     rec, m, rec_stride, rec_radii, overlap, ref_centroid, out);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_pose_contacts launch");
  return 0;
}
