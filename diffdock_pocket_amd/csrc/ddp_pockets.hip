// ddp_pockets.hip - geometric pocket finder on a grid (gfx950): occupancy of the protein's heavy atoms, LIGSITE-style buriedness, and
// the 6-connected components of the buried free points.  The definition is stated in include/ddp_hip.h and, in full, in
// diffdock_pocket_amd/pockets.py; the compaction of the pocket points uses ddp_select_jobs (ddp_lists.hip), and grouping, ranking and
// the centres are host work on that short list.  The reference has no counterpart: it takes the pocket centre from outside.
//
// Everything here is bitwise deterministic: occupancy stores the constant 1 (the order of concurrent stores cannot show), buriedness is
// a pure function of the occupancy grid, and a label is the smallest flat index of its component whatever the order of the atomics
// (ddp_pockets_uf.h).  No float atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_pockets_uf.h"

static int pockets_launch_ok(const char* what) {
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : ddp_fail_hip(err, what);
}

static bool grid_ok(int nx, int ny, int nz) {
  return nx > 0 && ny > 0 && nz > 0 && (long long)nx * ny * nz < (1ll << 31);
}

// ------------------------------------------------------------------------------------------------ occupancy
// index range [i0, i1] of one axis that the sphere can reach, clipped to [0, n - 1] (empty: i1 < i0).  Two points of slack on each
// side: the range only has to CONTAIN every point that passes the exact test below, and the fp32 rounding of these few operations
// is orders of magnitude below one grid step.  Clamped as floats before the conversion, so a far-away atom cannot overflow an int.
__device__ __forceinline__ void axis_range(float p, float lo, float inv_s, float reach, int n, int& i0, int& i1) {
  const float c = (p - lo) * inv_s;
  const float a = floorf(c - reach) - 2.0f, b = ceilf(c + reach) + 2.0f;
  i0 = (int)fminf(fmaxf(a, 0.0f), (float)n);
  i1 = (int)fminf(fmaxf(b, -1.0f), (float)(n - 1));
}

__global__ __launch_bounds__(256) void ddp_pocket_occupancy_kernel(const float* __restrict__ pos, const float* __restrict__ r2, int n_atoms,
                                                                   float lo_x, float lo_y, float lo_z, float s, int nx, int ny, int nz,
                                                                   uint8_t* __restrict__ occ) {
#pragma clang fp contract(off)
  const int atom = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (atom >= n_atoms) return;
  const float px = pos[3 * (size_t)atom], py = pos[3 * (size_t)atom + 1], pz = pos[3 * (size_t)atom + 2], rr = r2[atom];
  if (!(rr > 0.0f) || !(px == px) || !(py == py) || !(pz == pz)) return;   // nothing passes d2 < r2
  const float inv_s = 1.0f / s, reach = sqrtf(rr) * inv_s;
  int i0, i1, j0, j1, k0, k1;
  axis_range(px, lo_x, inv_s, reach, nx, i0, i1);
  axis_range(py, lo_y, inv_s, reach, ny, j0, j1);
  axis_range(pz, lo_z, inv_s, reach, nz, k0, k1);
  const int ci = i1 - i0 + 1, cj = j1 - j0 + 1, ck = k1 - k0 + 1;
  if (ci <= 0 || cj <= 0 || ck <= 0) return;
  const int cells = ci * cj * ck;      // <= nx ny nz < 2^31
  for (int t = lane; t < cells; t += 64) {
    const int k = k0 + t % ck, j = j0 + (t / ck) % cj, i = i0 + t / (ck * cj);     // inside [0, n) on every axis by the clipping
    const float xg = lo_x + (float)i * s, yg = lo_y + (float)j * s, zg = lo_z + (float)k * s;
    const float dx = xg - px, dy = yg - py, dz = zg - pz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float d2 = (xx + yy) + zz;
    if (d2 < rr) occ[((size_t)i * ny + j) * nz + k] = 1;
  }
}

extern "C" int ddp_pocket_occupancy(const float* pos, const float* r2, int n_atoms, float lo_x, float lo_y, float lo_z, float spacing, int nx,
                                    int ny, int nz, uint8_t* occ, void* stream) {
  if (!pos || !r2 || !occ) return ddp_fail(DDP_EINVAL, "ddp_pocket_occupancy: null argument");
  if (n_atoms <= 0 || !grid_ok(nx, ny, nz)) return ddp_fail(DDP_EINVAL, "ddp_pocket_occupancy: n_atoms <= 0, a dimension <= 0 or a grid of 2^31 points");
  if (!(spacing > 0.0f) || !isfinite(spacing) || !isfinite(lo_x) || !isfinite(lo_y) || !isfinite(lo_z))
    return ddp_fail(DDP_EINVAL, "ddp_pocket_occupancy: spacing <= 0 or a non-finite origin");
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(occ, 0, (size_t)nx * ny * nz, st);
  if (e != hipSuccess) return ddp_fail_hip(e, "ddp_pocket_occupancy memset");
  hipLaunchKernelGGL(ddp_pocket_occupancy_kernel, dim3((n_atoms + 3) / 4), dim3(256), 0, st, pos, r2, n_atoms, lo_x, lo_y, lo_z, spacing,
                     nx, ny, nz, occ);
  return pockets_launch_ok("ddp_pocket_occupancy launch");
}

// ------------------------------------------------------------------------------------------------ buriedness
__device__ __forceinline__ bool ray_hits(const uint8_t* __restrict__ occ, int nx, int ny, int nz, int i, int j, int k, int dx, int dy, int dz,
                                         int steps) {
  for (int t = 1; t <= steps; ++t) {
    i += dx;
    j += dy;
    k += dz;
    if (i < 0 || i >= nx || j < 0 || j >= ny || k < 0 || k >= nz) return false;      // outside the grid is free space
    if (occ[((size_t)i * ny + j) * nz + k]) return true;
  }
  return false;
}

__global__ __launch_bounds__(256) void ddp_pocket_buriedness_kernel(const uint8_t* __restrict__ occ, int nx, int ny, int nz, int n_axis,
                                                                    int n_diag, int min_lines, uint8_t* __restrict__ bur,
                                                                    int32_t* __restrict__ mask) {
  const int n = nx * ny * nz;
  const int g = blockIdx.x * 256 + (int)threadIdx.x;
  if (g >= n) return;
  if (occ[g]) {
    bur[g] = 0;
    mask[g] = 0;
    return;
  }
  const int k = g % nz, j = (g / nz) % ny, i = g / (nz * ny);
  const int dir[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};
  int count = 0;
#pragma unroll
  for (int l = 0; l < 7; ++l) {
    const int steps = l < 3 ? n_axis : n_diag;
    if (ray_hits(occ, nx, ny, nz, i, j, k, dir[l][0], dir[l][1], dir[l][2], steps) &&
        ray_hits(occ, nx, ny, nz, i, j, k, -dir[l][0], -dir[l][1], -dir[l][2], steps))
      ++count;
  }
  bur[g] = (uint8_t)count;
  mask[g] = count >= min_lines ? count + 1 : 0;
}

extern "C" int ddp_pocket_buriedness(const uint8_t* occ, int nx, int ny, int nz, double spacing, double ray_length, int min_lines,
                                     uint8_t* bur, int32_t* mask, void* stream) {
  if (!occ || !bur || !mask) return ddp_fail(DDP_EINVAL, "ddp_pocket_buriedness: null argument");
  if (!grid_ok(nx, ny, nz)) return ddp_fail(DDP_EINVAL, "ddp_pocket_buriedness: a dimension <= 0 or a grid of 2^31 points");
  if (!(spacing > 0.0) || !isfinite(spacing) || !(ray_length >= 0.0) || !isfinite(ray_length) || min_lines < 0 || min_lines > 7)
    return ddp_fail(DDP_EINVAL, "ddp_pocket_buriedness: spacing <= 0, ray_length < 0 or min_lines outside [0, 7]");
  // a ray longer than the grid leaves it anyway: the clamp only keeps the step counts inside an int
  const double cap = (double)(nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz));
  const int n_axis = (int)fmin(floor(ray_length / spacing), cap), n_diag = (int)fmin(floor(ray_length / (spacing * sqrt(3.0))), cap);
  const int n = nx * ny * nz;
  hipLaunchKernelGGL(ddp_pocket_buriedness_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, occ, nx, ny, nz, n_axis, n_diag,
                     min_lines, bur, mask);
  return pockets_launch_ok("ddp_pocket_buriedness launch");
}

// ------------------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(256) void ddp_pocket_label_init_kernel(const int32_t* __restrict__ mask, int n, int32_t* __restrict__ parent) {
  const int g = blockIdx.x * 256 + (int)threadIdx.x;
  if (g < n) parent[g] = mask[g] != 0 ? g : -1;
}

// every 6-neighbour edge once: from its end with the smaller flat index
__global__ __launch_bounds__(256) void ddp_pocket_label_union_kernel(const int32_t* __restrict__ mask, int nx, int ny, int nz,
                                                                     int32_t* parent) {
  const int n = nx * ny * nz;
  const int g = blockIdx.x * 256 + (int)threadIdx.x;
  if (g >= n || mask[g] == 0) return;
  const int k = g % nz, j = (g / nz) % ny, i = g / (nz * ny);
  if (k + 1 < nz && mask[g + 1] != 0) uf_union(parent, g, g + 1);
  if (j + 1 < ny && mask[g + nz] != 0) uf_union(parent, g, g + nz);
  if (i + 1 < nx && mask[g + ny * nz] != 0) uf_union(parent, g, g + ny * nz);
}

// parent[g] = root(g).  Concurrent with other threads' walks: a walk that meets an already flattened entry is only shorter.
__global__ __launch_bounds__(256) void ddp_pocket_label_flatten_kernel(int n, int32_t* parent) {
  const int g = blockIdx.x * 256 + (int)threadIdx.x;
  if (g >= n) return;
  const int32_t p = uf_load(parent + g);
  if (p < 0 || p == g) return;
  const int32_t r = uf_find(parent, p);
  if (r != p) __hip_atomic_store(parent + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern "C" int ddp_pocket_label(const int32_t* mask, int nx, int ny, int nz, int32_t* labels, void* stream) {
  if (!mask || !labels) return ddp_fail(DDP_EINVAL, "ddp_pocket_label: null argument");
  if (!grid_ok(nx, ny, nz)) return ddp_fail(DDP_EINVAL, "ddp_pocket_label: a dimension <= 0 or a grid of 2^31 points");
  const int n = nx * ny * nz;
  const dim3 grid((n + 255) / 256), block(256);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ddp_pocket_label_init_kernel, grid, block, 0, st, mask, n, labels);
  hipLaunchKernelGGL(ddp_pocket_label_union_kernel, grid, block, 0, st, mask, nx, ny, nz, labels);
  hipLaunchKernelGGL(ddp_pocket_label_flatten_kernel, grid, block, 0, st, n, labels);
  return pockets_launch_ok("ddp_pocket_label launch");
}
