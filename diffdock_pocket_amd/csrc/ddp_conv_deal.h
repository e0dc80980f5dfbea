// ddp_conv_deal.h - the order in which the workgroups of a conv launch take its tiles: one function for the kernels (conv_tile of
// ddp_conv_common.h) and for the host (ddp_conv_deal_tile of ddp_capi.hip, which the tests call).
#ifndef DDP_CONV_DEAL_H
#define DDP_CONV_DEAL_H
#include <hip/hip_runtime.h>

// workgroup id -> tile.  Workgroup ids are dealt round-robin to the 8 XCDs (each with its own L2): XCD x runs the ids with id % 8 == x.
// Neighbouring tiles share source nodes (G rows, x rows) and all tiles of a conv share its packed weights, so an XCD is given RUNS of
// consecutive tiles.  A workgroup's cost depends on its conv (the G runs per wave follow the edges per source node), so the runs are
// short and dealt in turn: the task-major tile list is cut into chunks of c tiles, chunk m goes to XCD m % 8 - every XCD receives the
// same mix of every conv of the launch, and all XCDs walk one conv's weight stream at the same time.  Inside the whole super-rows of 8 c
// tiles: id = 8 j + x -> tile ((j / c) 8 + x) c + j % c.  The tiles behind them (all of a launch of fewer than 8 c tiles; and c = 0:
// the whole launch) get one contiguous range per XCD: ntl = 8 q + rem tiles, XCD x takes q + (x < rem) of them.  A bijection of
// [0, total) for every total >= 1 (tests/test_conv_deal_cpu.py through ddp_conv_deal_tile).
__host__ __device__ __forceinline__ int ddp_xcd_range_tile(int id, int ntl) {
  const int q = ntl >> 3, rem = ntl & 7, x = id & 7;
  return ((x < rem) ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + (id >> 3);
}
__host__ __device__ __forceinline__ int ddp_deal_tile(int id, int total, int c) {
  if (c <= 0) return ddp_xcd_range_tile(id, total);
  const int whole = total - total % (8 * c);     // a multiple of 8: id & 7 names the XCD behind it too
  if (id >= whole) return whole + ddp_xcd_range_tile(id - whole, total - whole);
  const int x = id & 7, j = id >> 3, m = j / c;
  return (m * 8 + x) * c + (j - m * c);
}

#endif /* DDP_CONV_DEAL_H */
