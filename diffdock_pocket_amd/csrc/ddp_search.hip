// ddp_search.hip - iterated local search around sampled poses in the Vinardo-form score (include/ddp_hip.h, ddp_pose_search and
// ddp_pose_search_select; host side diffdock_pocket_amd/search.py, whose module docstring states the whole definition).
// The fused minimiser runs one workgroup per pose and leaves most of the chip idle; here every pose seeds `replicas` independent
// chains and every chain is a workgroup of its own, so the replicas run beside each other instead of after each other.  One
// 256-thread workgroup per row q = s replicas + r runs all cycles of the call.  Per cycle: the start pose is the pose map of
// ddp_pose_update applied to the row's current pose with the cycle's random move (mz_pose_update of ddp_minimize_loop.h, the move's
// torsion steps in the tile's first floats exactly as the descent's are); mz_descend of the same header runs the line search from it,
// which is the loop of ddp_pose_minimize_kernel, so a cycle's descent equals ddp_pose_minimize from the start pose bit for bit; the
// Metropolis decision and the best-so-far test are taken by every thread from the same words (the energies of the loop, which come
// from LDS behind a barrier, and the row's uniform random number), so they are workgroup-uniform.
// The current and the best pose live in the row's global state, not in LDS (the LDS plan is the minimiser's): the current pose is read
// into the pose buffer at the start of a cycle, the local minimum is written to cur_pos / best_pos only on a move or an improvement,
// and a barrier separates such a write from the next cycle's read.  The random numbers are inputs; there is no device RNG, no atomics,
// every sum has a fixed order.  No data-dependent control flow around a barrier: the conditions that skip one (replica 0 at cycle 0,
// n_tor = 0) are the same for all 256 threads, and a NaN pose takes the same path as every other.
#include "ddp_minimize_loop.h"

__global__ __launch_bounds__(DDP_MZ_THREADS) void ddp_pose_search_kernel(const ddp_search_args_t A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mz_lds[];
  const ddp_minimize_args_t& M = A.min;
  const int tid = threadIdx.x, n = M.n, T = M.n_tor, R = A.replicas;
  const size_t q = blockIdx.x, rows = (size_t)M.n_samples * R;
  const int s = (int)(q / R), r = (int)(q % R);
  const MzLds L = mz_carve(mz_lds, n);
  const float* __restrict__ as = M.anchor + (size_t)s * n * 3;     // the sampled pose: anchor of every replica
  const float* __restrict__ rs = M.rec + (size_t)s * M.rec_stride;
  float* xc = A.cur_pos + q * n * 3;
  float* xb = A.best_pos + q * n * 3;
  for (int i = tid; i < n; i += DDP_MZ_THREADS) { L.rad[i] = M.lig_radii[i]; L.lflag[i] = M.lig_flags[i]; }
  // the row's state, held by every thread: fresh (written here) or as the previous call left it
  double ec[4], eb[4];
  int best_cycle, accepted;
  if (A.cycle0 == 0) {
    for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) { const float v = as[i]; xc[i] = v; xb[i] = v; }
    for (int k = 0; k < 4; ++k) ec[k] = eb[k] = (double)INFINITY;
    best_cycle = -1;
    accepted = 0;
  } else {
    for (int k = 0; k < 4; ++k) { ec[k] = A.cur_e[4 * q + k]; eb[k] = A.best_e[4 * q + k]; }
    best_cycle = A.best_cycle[q];
    accepted = A.accepted[q];
  }
  __syncthreads();
  for (int c = 0; c < A.cycles; ++c) {
    const size_t cq = (size_t)c * rows + q;
    // 1. the start pose, into the trial buffer of the loop.  A thread reads the elements of xc that it wrote itself (the same
    // stride everywhere), and the barrier at the end of the previous cycle lies in between.
    if (r == 0 && A.cycle0 + c == 0) {
      for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) L.x[3 * n + i] = xc[i];
      __syncthreads();
    } else {
      const float* __restrict__ pt = A.perturb + cq * (size_t)(6 + T);
      for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) L.x[i] = xc[i];
      for (int j = tid; j < T; j += DDP_MZ_THREADS) ((float*)L.tile)[j] = pt[6 + j];
      const float tr[3] = {pt[0], pt[1], pt[2]}, rot[3] = {pt[3], pt[4], pt[5]};
      __syncthreads();
      mz_pose_update(M, L, L.x, L.x + 3 * n, tr, rot);
    }
    if (A.starts) {
      float* so = A.starts + cq * n * 3;
      for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) so[i] = L.x[3 * n + i];
    }
    // 2. the descent: the minimiser's loop from the start pose
    int cur = 0, taken = 0;
    double step = A.step_init;
    double el[4] = {0.0, 0.0, 0.0, 0.0}, e0[4] = {0.0, 0.0, 0.0, 0.0};
    mz_descend(M, L, rs, as, M.iterations, cur, step, taken, el, e0, (double*)nullptr, (size_t)0);
    // 3. Metropolis and 4. best, fp64; a NaN makes every comparison false
    const double u = A.u[cq];
    const bool move = (el[3] < ec[3]) || (u < exp(-(el[3] - ec[3]) / A.temperature));
    const bool improved = el[3] < eb[3];
    const float* xl = L.x + cur * 3 * n;
    if (move) {
      for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) xc[i] = xl[i];
      for (int k = 0; k < 4; ++k) ec[k] = el[k];
    }
    if (improved) {
      for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) xb[i] = xl[i];
      for (int k = 0; k < 4; ++k) eb[k] = el[k];
      best_cycle = A.cycle0 + c;
    }
    accepted += taken;
    // 5. record
    if (tid == 0) {
      A.trace[2 * cq] = e0[3];
      A.trace[2 * cq + 1] = el[3];
      A.flags[cq] = (uint8_t)((move ? 1 : 0) | (improved ? 2 : 0));
    }
    __syncthreads();                             // xl has been copied out before the next cycle stages a pose over it
  }
  if (tid == 0) {
    for (int k = 0; k < 4; ++k) { A.cur_e[4 * q + k] = ec[k]; A.best_e[4 * q + k] = eb[k]; }
    A.best_cycle[q] = best_cycle;
    A.accepted[q] = accepted;
  }
}

// one block per pose: the replica with the smallest best_e[.][3], strict < in replica order (a tie goes to the lower replica, NaN and
// +inf are never smaller; none smaller than +inf: replica 0).  Every thread runs the same scan over the same words.
__global__ __launch_bounds__(DDP_MZ_THREADS) void ddp_pose_search_select_kernel(const ddp_search_select_args_t A) {
  const int s = blockIdx.x, tid = threadIdx.x, n = A.n, R = A.replicas;
  int best = 0;
  double bv = (double)INFINITY;
  for (int r = 0; r < R; ++r) {
    const double v = A.best_e[4 * ((size_t)s * R + r) + 3];
    if (v < bv) { bv = v; best = r; }
  }
  const size_t q = (size_t)s * R + best;
  const float* __restrict__ src = A.best_pos + q * n * 3;
  float* dst = A.pos_out + (size_t)s * n * 3;
  for (int i = tid; i < 3 * n; i += DDP_MZ_THREADS) dst[i] = src[i];
  if (tid == 0) {
    for (int k = 0; k < 4; ++k) A.energy_out[4 * (size_t)s + k] = A.best_e[4 * q + k];
    A.replica_out[s] = best;
    A.cycle_out[s] = A.best_cycle[q];
  }
}

extern "C" int ddp_pose_search(const ddp_search_args_t* a, void* stream) {
  const char* who = "ddp_pose_search";
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_pose_search: null argument struct");
  const ddp_minimize_args_t* m = &a->min;
  if (m->n_samples == 0) return 0;
  if (const int rc = ddp_pose_check_shape(who, m->n_samples, m->n, m->m, m->rec_stride, m->n_tor >= 0)) return rc;
  if (const int rc = DDP_POSE_CHECK_ATOMS(who, m->n, DDP_MINIMIZE_MAX_ATOMS)) return rc;
  if (m->n_tor > DDP_MINIMIZE_MAX_TORSIONS) return ddp_fail(DDP_ELIMIT, "ddp_pose_search: more than DDP_MINIMIZE_MAX_TORSIONS rotatable bonds");
  if (!m->anchor || !m->lig_radii || !m->lig_flags || (m->m > 0 && (!m->rec || !m->rec_radii || !m->rec_flags)) ||
      (m->n_tor > 0 && (!m->bonds || !m->mask_rotate)))
    return ddp_fail(DDP_EINVAL, "ddp_pose_search: null argument");
  if (const int rc = ddp_pose_check_chain(who, a, m->n_samples, true,
                                          m->iterations < 0 || !(m->restraint >= 0.0) ? "iterations or restraint < 0" : nullptr))
    return rc;
  if (const int rc = score_check_constants(&m->form, who)) return rc;
  if (a->cycles == 0) return 0;
  hipLaunchKernelGGL(ddp_pose_search_kernel, dim3((unsigned)(m->n_samples * a->replicas)), dim3(DDP_MZ_THREADS), mz_lds_bytes(m->n),
                     (hipStream_t)stream, *a);
  return ddp_launch_result(who);
}

extern "C" int ddp_pose_search_select(const ddp_search_select_args_t* a, void* stream) {
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_pose_search_select: null argument struct");
  if (a->n_samples == 0) return 0;
  if (a->n_samples < 0 || a->n <= 0 || a->replicas < 1) return ddp_fail(DDP_EINVAL, "ddp_pose_search_select: shape");
  if (!a->best_pos || !a->best_e || !a->best_cycle || !a->pos_out || !a->energy_out || !a->replica_out || !a->cycle_out)
    return ddp_fail(DDP_EINVAL, "ddp_pose_search_select: null argument");
  hipLaunchKernelGGL(ddp_pose_search_select_kernel, dim3(a->n_samples), dim3(DDP_MZ_THREADS), 0, (hipStream_t)stream, *a);
  return ddp_launch_result("ddp_pose_search_select");
}
