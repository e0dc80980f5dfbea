// ddp_eval.hip - evaluation of sampled poses against a reference pose (include/ddp_hip.h, ddp_pose_rmsd / ddp_pose_contacts) and
// against each other (ddp_pose_pairwise_rmsd, ddp_pose_cluster):
//   symmetry-corrected RMSD (spyrmsd symmrmsd as called by utils/utils.py:116-130: no centring, no alignment, minimum over the
//   graph automorphisms), plain and side-chain RMSD (evaluate_files.py:150-154,237), centroid distance, minimum ligand-receptor /
//   ligand-ligand distances (evaluate_files.py:251-256) and the receptor-ligand steric-clash count (datasets/steric_clash.py:99-136).
// One 256-thread workgroup per sample (pairwise: per pose and tile of later poses; clustering: one workgroup), coordinates staged in LDS.  Every reduction is a fixed tree (wave shuffles, then the 4 waves
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

// ---- all pairs: dist[i][j] = dist[j][i] = what ddp_pose_rmsd gives sample j against ref = the n selected rows of pose i (i < j), bit for bit:
// the same fp32 differences, the same fp64 sum over atoms in increasing order, the same lane walk p = t, t + 256, ... and the same
// reduction tree.  Workgroup (i, tile) holds pose i and the T poses j0 .. j0 + T - 1, j0 = i + 1 + tile * T, in LDS; a lane loads each
// perms[a][p] once and feeds T fp64 accumulators from it, so the table is read once per tile instead of once per pair and direction.
// LDS image: x [n][T][3] (atom a of the T poses is one 12 T-byte row: vector reads, the same address in every lane), then r [n][3]
// (pose i, gathered through the permutation).  The last tile of a row is ragged: its missing poses are zeros and are not written.
template <int T>
__global__ __launch_bounds__(DDP_EVAL_THREADS) void ddp_pose_pairwise_rmsd_kernel(const float* __restrict__ pos, int S, int pos_stride,
                                                                                 const int32_t* __restrict__ sel, int n,
                                                                                 const int32_t* __restrict__ perms, int P,
                                                                                 float* __restrict__ dist) {
  extern __shared__ float4 pair_lds[];
  float* x = (float*)pair_lds;       // [n][T][3]
  float* r = x + 3 * T * n;          // [n][3]
  __shared__ double wv[T][DDP_EVAL_WAVES];
  __shared__ int wp[T][DDP_EVAL_WAVES];
  __shared__ int bad_sel;
  const int i = blockIdx.x, j0 = i + 1 + (int)blockIdx.y * T, tid = threadIdx.x;
  if (blockIdx.y == 0 && tid == 0) dist[(size_t)i * S + i] = 0.f;
  if (j0 >= S) return;               // right of the last pose: this row has fewer tiles than the longest one
  const int nt = min(T, S - j0);
  if (tid == 0) bad_sel = 0;
  __syncthreads();
  for (int k = tid; k < (T + 1) * n; k += DDP_EVAL_THREADS) {
    const int t = k / n, a = k - t * n;                  // t = 0: pose i, t >= 1: pose j0 + t - 1
    float* dst = t == 0 ? r + 3 * a : x + 3 * (a * T + t - 1);
    dst[0] = dst[1] = dst[2] = 0.f;
    if (t > nt) continue;
    const int row = sel ? sel[a] : a;
    if (row < 0 || 3 * row + 2 >= pos_stride) {          // a selected row outside the sample's row: no read, every pair gets NaN
      bad_sel = 1;
      continue;
    }
    const float* __restrict__ ps = pos + (size_t)(t == 0 ? i : j0 + t - 1) * pos_stride + 3 * row;
    dst[0] = ps[0]; dst[1] = ps[1]; dst[2] = ps[2];
  }
  __syncthreads();
  if (bad_sel) {
    if (tid < nt) dist[(size_t)i * S + j0 + tid] = dist[(size_t)(j0 + tid) * S + i] = __builtin_nanf("");
    return;
  }
  double bv[T];
  int bp[T];
#pragma unroll
  for (int t = 0; t < T; ++t) { bv[t] = 0.0; bp[t] = -1; }
  for (int p = tid; p < P; p += DDP_EVAL_THREADS) {
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    bool ok = true;
    for (int a = 0; a < n; ++a) {
      const int q = perms[(size_t)a * P + p];
      if (q < 0 || q >= n) { ok = false; break; }        // an entry outside [0, n): this permutation is not considered
      const float rx = r[3 * q], ry = r[3 * q + 1], rz = r[3 * q + 2];
      float xa[3 * T];
      if constexpr ((3 * T) % 4 == 0) {
        const float4* __restrict__ src = (const float4*)(x + 3 * T * a);
#pragma unroll
        for (int k = 0; k < 3 * T / 4; ++k) { const float4 v = src[k]; xa[4 * k] = v.x; xa[4 * k + 1] = v.y; xa[4 * k + 2] = v.z; xa[4 * k + 3] = v.w; }
      } else {
        const float2* __restrict__ src = (const float2*)(x + 3 * T * a);
#pragma unroll
        for (int k = 0; k < 3 * T / 2; ++k) { const float2 v = src[k]; xa[2 * k] = v.x; xa[2 * k + 1] = v.y; }
      }
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float dx = xa[3 * t] - rx, dy = xa[3 * t + 1] - ry, dz = xa[3 * t + 2] - rz;
        acc[t] += (double)dx * dx + (double)dy * dy + (double)dz * dz;
      }
    }
    if (ok) {
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (better(acc[t], p, bv[t], bp[t])) { bv[t] = acc[t]; bp[t] = p; }
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv[t], off);
      const int op = __shfl_xor(bp[t], off);
      if (better(ov, op, bv[t], bp[t])) { bv[t] = ov; bp[t] = op; }
    }
    if ((tid & 63) == 0) { wv[t][tid >> 6] = bv[t]; wp[t][tid >> 6] = bp[t]; }
  }
  __syncthreads();
  if (tid < nt) {                    // lane t finishes pose j0 + t: waves in increasing order, as lane 0 of ddp_pose_rmsd does
    double v = wv[tid][0];
    int p = wp[tid][0];
    for (int w = 1; w < DDP_EVAL_WAVES; ++w)
      if (better(wv[tid][w], wp[tid][w], v, p)) { v = wv[tid][w]; p = wp[tid][w]; }
    const float d = p >= 0 ? (float)sqrt(v / (double)n) : __builtin_nanf("");
    dist[(size_t)i * S + j0 + tid] = d;                  // the mirror is a copy: the other direction sums in another order
    dist[(size_t)(j0 + tid) * S + i] = d;
  }
}

// tile width from n: (T + 1) * 12 n bytes of LDS stay below 40 KiB (four workgroups per CU by LDS) and the widest tile goes to the
// small ligands, where the table is the cost.  Registers: 75 / 43 / 27 VGPRs at T = 8 / 4 / 2, six or more workgroups per CU.
static int pairwise_tile(int n) { return n <= 256 ? 8 : n <= 512 ? 4 : 2; }

template <int T>
static void launch_pairwise(const float* pos, int S, int pos_stride, const int32_t* sel, int n, const int32_t* perms, int P, float* dist,
                            hipStream_t stream) {
  const int tiles = S > 1 ? (S - 1 + T - 1) / T : 1;
  const size_t lds = (size_t)3 * (T + 1) * n * sizeof(float);
  hipLaunchKernelGGL(ddp_pose_pairwise_rmsd_kernel<T>, dim3(S, tiles), dim3(DDP_EVAL_THREADS), lds, stream, pos, S, pos_stride, sel, n,
                     perms, P, dist);
}

extern "C" int ddp_pose_pairwise_rmsd(const float* pos, int n_samples, int pos_stride, const int32_t* sel, int n, const int32_t* perms,
                                      int n_perms, float* dist, void* stream) {
  if (n_samples == 0) return 0;
  if (n_samples < 0 || n <= 0 || n_perms <= 0 || pos_stride < 3) return ddp_fail(DDP_EINVAL, "ddp_pose_pairwise_rmsd: shape");
  if (!pos || !perms || !dist) return ddp_fail(DDP_EINVAL, "ddp_pose_pairwise_rmsd: null argument");
  if (!sel && 3 * n > pos_stride) return ddp_fail(DDP_EINVAL, "ddp_pose_pairwise_rmsd: n rows do not fit in pos_stride");
  if (n > DDP_EVAL_MAX_ATOMS) return ddp_fail(DDP_ELIMIT, "ddp_pose_pairwise_rmsd: more than DDP_EVAL_MAX_ATOMS atoms");
  if (n_samples > DDP_PAIRWISE_MAX_SAMPLES) return ddp_fail(DDP_ELIMIT, "ddp_pose_pairwise_rmsd: more than DDP_PAIRWISE_MAX_SAMPLES samples");
  switch (pairwise_tile(n)) {
    case 8: launch_pairwise<8>(pos, n_samples, pos_stride, sel, n, perms, n_perms, dist, (hipStream_t)stream); break;
    case 4: launch_pairwise<4>(pos, n_samples, pos_stride, sel, n, perms, n_perms, dist, (hipStream_t)stream); break;
    default: launch_pairwise<2>(pos, n_samples, pos_stride, sel, n, perms, n_perms, dist, (hipStream_t)stream); break;
  }
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_pose_pairwise_rmsd launch");
  return 0;
}

// ---- greedy leader clustering on the matrix: one workgroup, lane t owns pose t.  Labels, representatives and sizes are built in LDS
// and leave in one pass at the end.  Each opened cluster costs a counting barrier (every lane has read the labels it needs, and gets
// the member count) and a plain one (the new labels are visible before the next entry of `order` is looked at).
#define DDP_CLUSTER_THREADS 1024
__global__ __launch_bounds__(DDP_CLUSTER_THREADS) void ddp_pose_cluster_kernel(const float* __restrict__ dist, int S,
                                                                              const int32_t* __restrict__ order, float cutoff,
                                                                              int32_t* __restrict__ labels, int32_t* __restrict__ reps,
                                                                              int32_t* __restrict__ sizes, int32_t* __restrict__ n_clusters) {
  __shared__ int lab[DDP_CLUSTER_THREADS], rep[DDP_CLUSTER_THREADS], cnt[DDP_CLUSTER_THREADS];
  const int t = threadIdx.x;
  lab[t] = rep[t] = cnt[t] = -1;
  __syncthreads();
  int nc = 0;
  for (int k = 0; k < S; ++k) {
    const int o = order ? order[k] : k;
    if (o < 0 || o >= S) continue;                       // not a pose: skipped, nothing is read
    if (lab[o] >= 0) continue;
    // strict <: a pose exactly at the cutoff stays out, NaN compares false; the representative is a member whatever its diagonal says
    const bool join = t < S && lab[t] < 0 && (t == o || dist[(size_t)o * S + t] < cutoff);
    const int members = __syncthreads_count(join);
    if (join) lab[t] = nc;
    if (t == 0) { rep[nc] = o; cnt[nc] = members; }
    ++nc;
    __syncthreads();
  }
  if (t < S) { labels[t] = lab[t]; reps[t] = rep[t]; sizes[t] = cnt[t]; }
  if (t == 0) *n_clusters = nc;
}

extern "C" int ddp_pose_cluster(const float* dist, int n_samples, const int32_t* order, float cutoff, int32_t* labels, int32_t* reps,
                                int32_t* sizes, int32_t* n_clusters, void* stream) {
  if (n_samples < 0) return ddp_fail(DDP_EINVAL, "ddp_pose_cluster: shape");
  if (n_samples > DDP_CLUSTER_THREADS) return ddp_fail(DDP_ELIMIT, "ddp_pose_cluster: more than 1024 samples");
  if (!n_clusters || (n_samples > 0 && (!dist || !labels || !reps || !sizes))) return ddp_fail(DDP_EINVAL, "ddp_pose_cluster: null argument");
  const int threads = n_samples > 64 ? (n_samples + 63) / 64 * 64 : 64;
  hipLaunchKernelGGL(ddp_pose_cluster_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, dist, n_samples, order, cutoff, labels, reps,
                     sizes, n_clusters);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_pose_cluster launch");
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
