// ddp_search_flex.hip - iterated local search around sampled poses TOGETHER with the flexible side chains of their receptor
// (include/ddp_hip.h, ddp_pose_search_flex; host side diffdock_pocket_amd/search_flex.py, whose module docstring states the whole
// definition).  The sibling of ddp_search.hip with the second molecule of ddp_minimize_flex.hip in the state: one 256-thread
// workgroup per row q = s replicas + r runs all cycles of the call.  Per cycle: the start state is the pose map of ddp_pose_update
// applied to the row's current ligand pose and the side-chain map of ddp_sidechain_update (fx_sc_update) applied to the row's current
// moving atoms, both with the cycle's random move (the torsion steps in the tile's first floats and the chi steps in L.scstep,
// exactly as the descent's are); fx_descend of ddp_minimize_flex_loop.h runs the joint line search from it, which is the loop of
// ddp_pose_minimize_flex_kernel, so a cycle's descent equals ddp_pose_minimize_flex from the start state bit for bit; the Metropolis
// decision and the best-so-far test are taken by every thread from the same words (the energies of the loop, which come from LDS
// behind a barrier, and the row's uniform random number), so they are workgroup-uniform.
// The current and the best state (ligand pose and the n_mov moving atoms, compact) live in the row's global state, not in LDS (the LDS
// plan is the joint minimiser's, unchanged): they are read into the current buffers at the start of a cycle, the local minimum is
// written to cur_* / best_* only on a move or an improvement, and a barrier separates such a write from the next cycle's read.  A
// thread reads back only the elements it wrote itself (the same stride everywhere).  The receptor rec + s rec_stride is READ ONLY: its
// moving atoms are read for the fresh state, every other atom throughout, so the replicas of a pose share it.  The random numbers are
// inputs; there is no device RNG, no atomics, every sum has a fixed order, every store is a plain vector store.  No data-dependent
// control flow around a barrier: the conditions that skip one (replica 0 at cycle 0, n_tor = 0, n_sc = 0, an index outside the
// receptor) are the same for all 256 threads, and a NaN state takes the same path as every other.
#include "ddp_minimize_flex_loop.h"

__global__ __launch_bounds__(DDP_FX_THREADS) void ddp_pose_search_flex_kernel(const ddp_search_flex_args_t A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fx_lds[];
  const ddp_minimize_flex_args_t& F = A.flex;
  const int tid = threadIdx.x, n = F.n, m = F.m, n_mov = F.n_mov, n_sc = F.n_sc, T = F.n_tor, R = A.replicas;
  const size_t q = blockIdx.x, rows = (size_t)F.n_samples * R;
  const int s = (int)(q / R), r = (int)(q % R);
  const FxLds L = fx_carve(fx_lds, n, n_mov, n_sc);
  const float* __restrict__ as = F.anchor + (size_t)s * n * 3;              // the sampled pose: anchor of every replica
  const float* __restrict__ rs = F.rec + (size_t)s * F.rec_stride;          // the sampled receptor, never written
  const float* __restrict__ ras = F.rec_anchor + (size_t)s * F.rec_stride;  // the side chains' anchor
  float* xc = A.cur_pos + q * n * 3;
  float* xb = A.best_pos + q * n * 3;
  float* yc = A.cur_mov + q * n_mov * 3;
  float* yb = A.best_mov + q * n_mov * 3;
  fx_load_tables(F, L);
  // the row's state, held by every thread: fresh (written here) or as the previous call left it
  double ec[6], eb[6];
  int best_cycle, accepted;
  if (A.cycle0 == 0) {
    for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) { const float v = as[i]; xc[i] = v; xb[i] = v; }
    for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) {
      const int a = F.mov[i / 3];
      const float v = (a >= 0 && a < m) ? rs[3 * a + i % 3] : 0.f;     // an index outside the receptor: no read
      yc[i] = v; yb[i] = v;
    }
    for (int k = 0; k < 6; ++k) ec[k] = eb[k] = (double)INFINITY;
    best_cycle = -1;
    accepted = 0;
  } else {
    for (int k = 0; k < 6; ++k) { ec[k] = A.cur_e[6 * q + k]; eb[k] = A.best_e[6 * q + k]; }
    best_cycle = A.best_cycle[q];
    accepted = A.accepted[q];
  }
  __syncthreads();
  for (int c = 0; c < A.cycles; ++c) {
    const size_t cq = (size_t)c * rows + q;
    // 1. the start state, into the trial buffers of the loop.  A thread reads the elements of xc and yc that it wrote itself, and the
    // barrier at the end of the previous cycle lies in between.
    if (r == 0 && A.cycle0 + c == 0) {
      for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) L.x[3 * n + i] = xc[i];
      for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) L.ym[3 * n_mov + i] = yc[i];
      __syncthreads();
    } else {
      const float* __restrict__ pt = A.perturb + cq * (size_t)(6 + T + n_sc);
      for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) L.x[i] = xc[i];
      for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) L.ym[i] = yc[i];
      for (int j = tid; j < T; j += DDP_FX_THREADS) ((float*)L.tile)[j] = pt[6 + j];
      for (int j = tid; j < n_sc; j += DDP_FX_THREADS) L.scstep[j] = pt[6 + T + j];
      const float tr[3] = {pt[0], pt[1], pt[2]}, rot[3] = {pt[3], pt[4], pt[5]};
      __syncthreads();
      descent_pose_update(F, L.x, L.x + 3 * n, L.rg, (const float*)L.tile, (float*)L.red, tr, rot);
      fx_sc_update(F, L, rs, L.ym, L.ym + 3 * n_mov);
    }
    if (A.starts) {
      float* so = A.starts + cq * n * 3;
      for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) so[i] = L.x[3 * n + i];
    }
    if (A.starts_mov) {
      float* so = A.starts_mov + cq * n_mov * 3;
      for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) so[i] = L.ym[3 * n_mov + i];
    }
    // 2. the descent: the joint minimiser's loop from the start state
    int cur = 0, taken = 0;
    double step = A.step_init;
    double el[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, e0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    fx_descend(F, L, rs, as, ras, F.iterations, cur, step, taken, el, e0, (double*)nullptr, (size_t)0);
    // 3. Metropolis and 4. best, fp64; a NaN makes every comparison false
    const double u = A.u[cq];
    const bool move = (el[5] < ec[5]) || (u < exp(-(el[5] - ec[5]) / A.temperature));
    const bool improved = el[5] < eb[5];
    const float* xl = L.x + cur * 3 * n;
    const float* yl = L.ym + cur * 3 * n_mov;
    if (move) {
      for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) xc[i] = xl[i];
      for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) yc[i] = yl[i];
      for (int k = 0; k < 6; ++k) ec[k] = el[k];
    }
    if (improved) {
      for (int i = tid; i < 3 * n; i += DDP_FX_THREADS) xb[i] = xl[i];
      for (int i = tid; i < 3 * n_mov; i += DDP_FX_THREADS) yb[i] = yl[i];
      for (int k = 0; k < 6; ++k) eb[k] = el[k];
      best_cycle = A.cycle0 + c;
    }
    accepted += taken;
    // 5. record
    if (tid == 0) {
      A.trace[2 * cq] = e0[5];
      A.trace[2 * cq + 1] = el[5];
      A.flags[cq] = (uint8_t)((move ? 1 : 0) | (improved ? 2 : 0));
    }
    __syncthreads();                             // xl and yl have been copied out before the next cycle stages a state over them
  }
  if (tid == 0) {
    for (int k = 0; k < 6; ++k) { A.cur_e[6 * q + k] = ec[k]; A.best_e[6 * q + k] = eb[k]; }
    A.best_cycle[q] = best_cycle;
    A.accepted[q] = accepted;
  }
}

extern "C" int ddp_pose_search_flex(const ddp_search_flex_args_t* a, void* stream) {
  const char* who = "ddp_pose_search_flex";
  if (!a) return ddp_fail(DDP_EINVAL, "ddp_pose_search_flex: null argument struct");
  const ddp_minimize_flex_args_t* f = &a->flex;
  if (f->n_samples == 0) return 0;
  if (const int rc = fx_check(who, f)) return rc;
  if (!f->anchor || !f->lig_radii || !f->lig_flags || (f->m > 0 && (!f->rec || !f->rec_radii || !f->rec_flags)) ||
      (f->n_tor > 0 && (!f->bonds || !f->mask_rotate)) || (f->n_mov > 0 && !f->rec_anchor))
    return ddp_fail(DDP_EINVAL, "ddp_pose_search_flex: null argument");
  if (const int rc = ddp_pose_check_chain(who, a, f->n_samples, f->n_mov == 0 || (a->cur_mov && a->best_mov),
                                          f->iterations < 0 || !(f->restraint >= 0.0) || !(f->restraint_sc >= 0.0)
                                              ? "iterations or a restraint < 0" : nullptr))
    return rc;
  if (const int rc = score_check_constants(&f->form, who)) return rc;
  if (a->cycles == 0) return 0;
  hipLaunchKernelGGL(ddp_pose_search_flex_kernel, dim3((unsigned)(f->n_samples * a->replicas)), dim3(DDP_FX_THREADS),
                     fx_lds_bytes(f->n, f->n_mov, f->n_sc), (hipStream_t)stream, *a);
  return ddp_launch_result(who);
}
