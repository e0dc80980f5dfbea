// ddp_traj.hip - reverse-process trajectory recording (include/ddp_hip.h, ddp_traj_record; host side sampler.py).
// The counterpart of the reference's per-sample, per-step `.cpu()` copies of the poses (inference.py:146-165 with
// --save_visualisation, the visualisation lists of utils/sampling.py, utils/visualise.py) for a denoising step that is replayed as
// one captured graph: the slot to write is read from device memory (the step's parameter block, written by the step's one
// host-to-device copy), so ONE captured launch serves every step.  Exact copies, no arithmetic: lane i of the grid moves float i of
// the step's record; the ligand part is a contiguous block per sample (coalesced in and out), the atom part gathers the moving atoms'
// three floats per row.  No atomics, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"

#define DDP_TRAJ_THREADS 256

__global__ __launch_bounds__(DDP_TRAJ_THREADS) void ddp_traj_record_kernel(const float* __restrict__ lig_pos, int n, int n_lig,
                                                                          float* __restrict__ lig_traj,
                                                                          const float* __restrict__ atom_pos, int n_atoms,
                                                                          const int32_t* __restrict__ moving, int n_moving,
                                                                          float* __restrict__ atom_traj, int n_slots,
                                                                          const float* __restrict__ slot) {
  const float fs = slot[0];
  if (!(fs >= 0.0f && fs < (float)n_slots)) return;       // (NaN included) a slot outside [0, n_slots): nothing is written
  const int k = (int)fs;
  const int64_t lig_row = 3 * (int64_t)n_lig, atom_row = 3 * (int64_t)n_moving;
  const int64_t n_lig_floats = (int64_t)n * lig_row;
  const int64_t total = n_lig_floats + (int64_t)n * atom_row;
  for (int64_t i = (int64_t)blockIdx.x * DDP_TRAJ_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * DDP_TRAJ_THREADS) {
    if (i < n_lig_floats) {
      const int64_t s = i / lig_row, j = i - s * lig_row;
      lig_traj[(s * n_slots + k) * lig_row + j] = lig_pos[i];
    } else {
      const int64_t q = i - n_lig_floats;
      const int64_t s = q / atom_row, j = q - s * atom_row;
      const int64_t m = j / 3, c = j - 3 * m;
      const int a = moving[m];
      if (a < 0 || a >= n_atoms) continue;                  // an index outside the sample's atoms: no read, no write
      atom_traj[(s * n_slots + k) * atom_row + j] = atom_pos[((int64_t)s * n_atoms + a) * 3 + c];
    }
  }
}

extern "C" int ddp_traj_record(const float* lig_pos, int n, int n_lig, float* lig_traj, const float* atom_pos, int n_atoms,
                               const int32_t* moving, int n_moving, float* atom_traj, int n_slots, const float* slot, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || n_lig <= 0 || n_slots <= 0 || n_moving < 0 || n_atoms < 0) return ddp_fail(DDP_EINVAL, "ddp_traj_record: shape");
  if (!lig_pos || !lig_traj || !slot) return ddp_fail(DDP_EINVAL, "ddp_traj_record: null argument");
  if (n_moving > 0 && (!atom_pos || !moving || !atom_traj || n_atoms <= 0))
    return ddp_fail(DDP_EINVAL, "ddp_traj_record: moving atoms without atom_pos / index list / atom_traj");
  const int64_t total = (int64_t)n * 3 * ((int64_t)n_lig + n_moving);
  const int64_t blocks = (total + DDP_TRAJ_THREADS - 1) / DDP_TRAJ_THREADS;
  const int grid = (int)(blocks < 1024 ? blocks : 1024);
  hipLaunchKernelGGL(ddp_traj_record_kernel, dim3(grid), dim3(DDP_TRAJ_THREADS), 0, (hipStream_t)stream, lig_pos, n, n_lig, lig_traj,
                     atom_pos, n_atoms, moving, n_moving, atom_traj, n_slots, slot);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_traj_record launch");
  return 0;
}
