// ddp_front_lists.hip - the pose-dependent edge lists of a step's front in two launches (include/ddp_hip.h: ddp_front_lists).
//
// In a batch every list of the front is per sample: the ligand, receptor and atom nodes of sample g are contiguous ranges, a
// search never crosses graphs and every grouping key is a node index inside the sample's range.  So every output array is the
// concatenation, sample after sample, of a small per-sample result, and ONE WORKGROUP PER SAMPLE can produce it:
//   masks   the sample's match matrices (ligand x ligand, ligand x receptor, ligand x atom, bond centre x ligand) as 64-bit
//           words in LDS, one ballot per (query, 64 points); the caps keep the first bits of a row
//   count   launch 1: popcounts -> one total per (sample, list) in `scratch`
//   fill    launch 2, five workgroups per sample (FL_PART_*): each rebuilds the masks its part needs (44 k distance evaluations
//           from LDS-resident queries, 20 us for all of them - a round trip of the words through memory saves none of the
//           parts' own time), sums the totals of the earlier samples for its offsets (n_graphs values per list, no scan launch)
//           and writes its part: the query-major lists, the row pointers, the views grouped by point (a thread per column walks
//           the queries: ascending query = ascending original index = the stable order), the source-ordered views.  As one
//           workgroup per sample the parts ran one behind the other, each a latency chain: 125 us against 20 for the count
// No workgroup waits for another: the only dependency is the boundary between the two launches.
// The distance arithmetic is csrc/ddp_radius_math.h, shared with the search kernels this replaces.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddp_hip.h"
#include "ddp_internal.h"
#include "ddp_radius_math.h"

#define FL_THREADS 1024
#define FL_WAVES (FL_THREADS / 64)
#define FL_NL DDP_FRONT_MAX_LIG
#define FL_WR (DDP_FRONT_MAX_REC / 64)
#define FL_WA (DDP_FRONT_MAX_ATOM / 64)
#define FL_NB DDP_FRONT_MAX_BONDS
// parts of the fill launch (blockIdx.y)
#define FL_PART_LISTS 0   // query-major ll, lr and torsion lists, their row pointers, the counts
#define FL_PART_LA 1      // query-major ligand x atom list, its row pointers
#define FL_PART_C_LA 2    // ligand x atom by atom, the near rows
#define FL_PART_C_LR 3    // ligand x receptor by residue
#define FL_PART_LL 4      // the ligand list by either end (bond entries + radius pairs)
#define FL_PARTS 5
static_assert(FL_NL == 64, "a ligand row of the masks is one 64-bit word");

typedef unsigned long long u64;

struct FrontLds {
  float lp[3 * FL_NL], lps[3 * FL_NL], tp[3 * FL_NL];   // ligand atoms, the same divided by the sample's cutoff, bond centres
  u64 mll[FL_NL], mtor[FL_NL], mlr[FL_NL * FL_WR], mla[FL_NL * FL_WA];
  unsigned short plr[FL_NL * FL_WR], pla[FL_NL * FL_WA];   // matches of the row in the words before this one
  int off[4][FL_NL + 1];                                 // 0 ll, 1 lr, 2 la, 3 tor: matches of the sample's rows before this one
  int wsum[FL_WAVES];
  int tot[8], base[8];                                   // per list: all samples / the samples before this one
  int nbond;
  int bl[FL_NB], bk0[FL_NB], bk1[FL_NB], posb[FL_NB];    // the sample's bond entries: index, local ends, position in c_ll
  int nb0[FL_NL], nb1[FL_NL], rs0[FL_NL], rs1[FL_NL];    // bond entries per node by either end, local row starts of c_ll / so_ll
  int posr[FL_NL * FL_NL];                               // position in c_ll of the radius pair (query, point)
};

__device__ __forceinline__ u64 bits_below(int b) { return (1ull << b) - 1ull; }

// the first `cap` set bits of a row: what the search keeps of a capped query (index order)
__device__ __forceinline__ u64 first_bits(u64 m, int cap) {
  while (__popcll(m) > cap) m &= ~(1ull << (63 - __clzll((long long)m)));
  return m;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// exclusive prefix of v over the workgroup's threads and the sum (every thread calls it)
__device__ int block_excl_scan(int v, int* wsum, int& total) {
  const int lane = (int)threadIdx.x & 63, wid = (int)threadIdx.x >> 6;
  const int incl = wave_incl_scan(v, lane);
  if (lane == 63) wsum[wid] = incl;
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < FL_WAVES; ++w) {
    const int t = wsum[w];
    tot += t;
    if (w < wid) pre += t;
  }
  __syncthreads();
  total = tot;
  return pre + incl - v;
}

__device__ __forceinline__ int clamp_count(int n, int cap) { return n < cap ? (n < 0 ? 0 : n) : cap; }

// A query-major list (rows = the sample's ligand atoms, W words per row) grouped by POINT: rowptr, perm, key, out0 of the view
// and, for the view's own regrouping by query (which restores the original order), the position of every pair in the view.
// Only the first n pairs of the whole list take part.  NEAR: also the compacted list of the columns with a match.
template <int W, bool NEAR>
__device__ void column_view(const u64* mask, const unsigned short* pre, const int* off, int nq, int ncols, int base, int n, int x0,
                            int q0, int n_nodes, bool last, const ddp_front_view_t& c, int32_t* so_perm, int* wsum,
                            int32_t* near_rows, int near_base) {
  const int tid = (int)threadIdx.x;
  const int rbase = base < n ? base : n;
  int carry = 0, ncarry = 0;
  for (int j0 = 0; j0 < ncols; j0 += FL_THREADS) {
    const int j = j0 + tid, w = j >> 6, b = j & 63;
    int cc = 0, tc = 0;
    if (j < ncols)
      for (int q = 0; q < nq; ++q) {
        const u64 m = mask[q * W + w];
        if ((m >> b) & 1ull) {
          ++tc;
          cc += (base + off[q] + (int)pre[q * W + w] + __popcll(m & bits_below(b))) < n ? 1 : 0;
        }
      }
    int total;
    const int ex = block_excl_scan(cc, wsum, total) + carry;
    if (j < ncols) {
      c.rowptr[x0 + j] = rbase + ex;
      int k = 0;
      for (int q = 0; q < nq && k < cc; ++q) {       // (ascending query = ascending original index: the first cc are inside n)
        const u64 m = mask[q * W + w];
        if ((m >> b) & 1ull) {
          const int orig = base + off[q] + (int)pre[q * W + w] + __popcll(m & bits_below(b));
          const int p = rbase + ex + k;
          c.perm[p] = orig;
          c.key[p] = x0 + j;
          c.out0[p] = q0 + q;
          so_perm[orig] = p;
          ++k;
        }
      }
    }
    carry += total;
    if (NEAR) {
      int ntot;
      const int ex2 = block_excl_scan(tc != 0 ? 1 : 0, wsum, ntot) + ncarry;
      if (j < ncols && tc != 0) near_rows[near_base + ex2] = x0 + j;
      ncarry += ntot;
    }
  }
  if (last)
    for (int i = x0 + ncols + tid; i <= n_nodes; i += FL_THREADS) c.rowptr[i] = n;
}

template <bool FILL>
__global__ __launch_bounds__(FL_THREADS) void ddp_front_lists_kernel(const ddp_front_lists_t A) {
  __shared__ FrontLds S;
  const int g = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // the fill launch runs five workgroups per sample, each with the masks its part needs (the parts are latency chains of their
  // own: side by side they take the longest one's time, one behind the other their sum)
  const int part = FILL ? (int)blockIdx.y : -1;
  const bool need_ll = !FILL || part == FL_PART_LISTS || part == FL_PART_LL, need_tor = !FILL || part == FL_PART_LISTS;
  const bool need_lr = !FILL || part == FL_PART_LISTS || part == FL_PART_C_LR, need_la = !FILL || part == FL_PART_LA || part == FL_PART_C_LA;
  const int l0 = A.lig_ptr[g], nl = A.lig_ptr[g + 1] - l0;
  const int r0 = A.rec_ptr[g], nr = A.rec_ptr[g + 1] - r0;
  const int a0 = A.atom_ptr[g], na = A.atom_ptr[g + 1] - a0;
  const bool tor = A.tor_pos != nullptr && A.n_tor > 0;
  const int t0 = tor ? A.tor_ptr[g] : 0, nt = tor ? A.tor_ptr[g + 1] - t0 : 0;
  // (the host entry has checked the largest sample it was told of - max_* are trusted; a sample beyond the LDS plan all the same
  // writes no list, and zero totals, so that the other samples' offsets are sums of defined values)
  if (nl < 0 || nl > FL_NL || nt < 0 || nt > FL_NL || nr < 0 || nr > DDP_FRONT_MAX_REC || na < 0 || na > DDP_FRONT_MAX_ATOM) {
    if (!FILL && tid < 8) A.scratch[8 * g + tid] = 0;
    return;
  }
  const bool scaled = A.cross_div != nullptr;
  const float div = scaled ? A.cross_div[g] : 1.f;
  const float r2l = A.r_lig * A.r_lig, r2c = A.r_cross * A.r_cross;

  for (int i = tid; i < nl; i += FL_THREADS) {
    load_pt(A.lig_pos, (size_t)(l0 + i), false, 1.f, &S.lp[3 * i]);
    load_pt(A.lig_pos, (size_t)(l0 + i), scaled, div, &S.lps[3 * i]);
  }
  for (int i = tid; i < nt; i += FL_THREADS) load_pt(A.tor_pos, (size_t)(t0 + i), false, 1.f, &S.tp[3 * i]);
  if (tid < 8) S.tot[tid] = S.base[tid] = 0;
  if (tid < FL_NL) S.nb0[tid] = S.nb1[tid] = 0;
  if (tid == 0) S.nbond = 0;
  __syncthreads();

  // ---- masks: a wave per 64 points, the lane keeps its point in registers and meets every query of the sample
  const int Wr = (nr + 63) >> 6, Wa = (na + 63) >> 6;
  for (int task = wid; task < 2 + Wr + Wa; task += FL_WAVES) {
    float xj[3] = {0.f, 0.f, 0.f};
    if (task == 0 ? !need_ll : task == 1 ? !need_tor : task < 2 + Wr ? !need_lr : !need_la) continue;
    if (task < 2) {                       // points = the ligand atoms; queries: the ligand atoms / the bond centres
      const bool valid = lane < nl;
      if (valid) { xj[0] = S.lp[3 * lane]; xj[1] = S.lp[3 * lane + 1]; xj[2] = S.lp[3 * lane + 2]; }
      if (task == 0) {
        for (int q = 0; q < nl; ++q) {
          const u64 mm = __ballot(valid && sqdist(&S.lp[3 * q], xj) < r2l);
          if (lane == 0) S.mll[q] = first_bits(mm, A.ll_neighbors) & ~(1ull << q);   // self counts towards the cap, then goes
        }
      } else {
        for (int q = 0; q < nt; ++q) {
          const u64 mm = __ballot(valid && sqdist(&S.tp[3 * q], xj) < r2l);
          if (lane == 0) S.mtor[q] = first_bits(mm, A.tor_neighbors);
        }
      }
    } else if (task < 2 + Wr) {
      const int w = task - 2, j = 64 * w + lane;
      const bool valid = j < nr;
      if (valid) load_pt(A.rec_pos, (size_t)(r0 + j), scaled, div, xj);
      for (int q = 0; q < nl; ++q) {
        const u64 mm = __ballot(valid && sqdist(&S.lps[3 * q], xj) < r2c);
        if (lane == 0) S.mlr[q * FL_WR + w] = mm;
      }
    } else {
      const int w = task - 2 - Wr, j = 64 * w + lane;
      const bool valid = j < na;
      if (valid) load_pt(A.atom_pos, (size_t)(a0 + j), false, 1.f, xj);
      int c = 0;
      for (int q = 0; q < nl; ++q) {
        const bool m = valid && sqdist(&S.lp[3 * q], xj) < r2l;
        const u64 mm = __ballot(m);
        c += m ? 1 : 0;
        if (lane == 0) S.mla[q * FL_WA + w] = mm;
      }
      if (!FILL) {                        // the role-swapped search's count: (a - b)^2 = (b - a)^2 exactly
        if (valid) A.touched[a0 + j] = c;
        const u64 nz = __ballot(c != 0);
        if (lane == 0) atomicAdd(&S.tot[4], __popcll(nz));
      }
    }
  }
  // the sample's bond entries (ll0 / ll1 [0, e_bond), written before this launch)
  for (int i = tid; i < (need_ll && part != FL_PART_LISTS ? A.e_bond : 0); i += FL_THREADS) {
    const int k = A.ll0[i] - l0;
    if ((unsigned)k < (unsigned)nl) {
      const int slot = atomicAdd(&S.nbond, 1);
      if (FILL && slot < FL_NB) S.bl[slot] = i;
    }
  }
  __syncthreads();

  // ---- row counts, their prefix inside the row's words and over the sample's rows (a wave per list)
  if (tid < 256) {
    const int q = lane;
    int c = 0;
    if (wid == 0) {
      if (q < nl) c = __popcll(S.mll[q]);
    } else if (wid == 1) {
      if (q < nl)
        for (int w = 0; w < Wr; ++w) { S.plr[q * FL_WR + w] = (unsigned short)c; c += __popcll(S.mlr[q * FL_WR + w]); }
    } else if (wid == 2) {
      if (q < nl)
        for (int w = 0; w < Wa; ++w) { S.pla[q * FL_WA + w] = (unsigned short)c; c += __popcll(S.mla[q * FL_WA + w]); }
    } else if (q < nt) {
      c = __popcll(S.mtor[q]);
    }
    const int incl = wave_incl_scan(c, lane);
    S.off[wid][q] = incl - c;
    if (lane == 63) S.off[wid][FL_NL] = incl;
  }
  __syncthreads();

  if (!FILL) {
    if (tid < 8) {
      int v = 0;
      if (tid < 4) v = S.off[tid][FL_NL];
      else if (tid == 4) v = S.tot[4];
      else if (tid == 5) v = S.nbond;
      A.scratch[8 * g + tid] = v;
    }
    return;
  }

  // ---- fill: the sample's offset in every list = the totals of the samples before it
  for (int idx = tid; idx < 8 * A.n_graphs; idx += FL_THREADS) {
    const int v = A.scratch[idx], s = idx & 7;
    if (v != 0) {
      atomicAdd(&S.tot[s], v);
      if ((idx >> 3) < g) atomicAdd(&S.base[s], v);
    }
  }
  __syncthreads();
  const int Eb = A.e_bond;
  const int n_ll = clamp_count(Eb + S.tot[0], A.cap_ll), n_lr = clamp_count(S.tot[1], A.cap_lr);
  const int n_la = clamp_count(S.tot[2], A.cap_la), n_tor = clamp_count(S.tot[3], A.cap_tor);
  const int b_ll = Eb + S.base[0], b_lr = S.base[1], b_la = S.base[2], b_tor = S.base[3], b_near = S.base[4], b_bond = S.base[5];
  const bool last = g == A.n_graphs - 1;
  if (g == 0 && tid == 0 && part == FL_PART_LISTS) {
    *A.cnt_ll = Eb + S.tot[0];
    *A.cnt_lr = S.tot[1];
    *A.cnt_la = S.tot[2];
    *A.cnt_near = S.tot[4];
    if (tor) *A.cnt_tor = S.tot[3];
  }

  // ---- the query-major lists (a wave per row, a lane per bit) and what regrouping a point-grouped view by query restores
  for (int row = wid; row < nl; row += FL_WAVES) {
    const int q = l0 + row;
    if (part == FL_PART_LISTS) {
      const u64 m = S.mll[row];
      if ((m >> lane) & 1ull) {
        const int o = b_ll + S.off[0][row] + __popcll(m & bits_below(lane));
        if (o < A.cap_ll) {
          A.ll1[o] = q;
          A.ll0[o] = l0 + lane;
        }
      }
    }
    for (int w = 0; w < (part == FL_PART_LISTS ? Wr : 0); ++w) {
      const u64 m = S.mlr[row * FL_WR + w];
      if ((m >> lane) & 1ull) {
        const int o = b_lr + S.off[1][row] + (int)S.plr[row * FL_WR + w] + __popcll(m & bits_below(lane));
        if (o < A.cap_lr) {
          const int x = r0 + 64 * w + lane;
          A.lr0[o] = q;
          A.lr1[o] = x;
          A.so_lr.key[o] = q;
          A.so_lr.out0[o] = x;
          A.so_lr.out1[o] = o;
        }
      }
    }
    for (int w = 0; w < (part == FL_PART_LA ? Wa : 0); ++w) {
      const u64 m = S.mla[row * FL_WA + w];
      if ((m >> lane) & 1ull) {
        const int o = b_la + S.off[2][row] + (int)S.pla[row * FL_WA + w] + __popcll(m & bits_below(lane));
        if (o < A.cap_la) {
          const int x = a0 + 64 * w + lane;
          A.la0[o] = q;
          A.la1[o] = x;
          A.so_la.key[o] = q;
          A.so_la.out0[o] = x;
          A.so_la.out1[o] = o;
        } else if (A.overflow) {
          *A.overflow = 1;
        }
      }
    }
  }
  for (int row = wid; row < (part == FL_PART_LISTS ? nt : 0); row += FL_WAVES) {
    const u64 m = S.mtor[row];
    if ((m >> lane) & 1ull) {
      const int o = b_tor + S.off[3][row] + __popcll(m & bits_below(lane));
      if (o < A.cap_tor) {
        A.tor_q[o] = t0 + row;
        A.tor_x[o] = l0 + lane;
      }
    }
  }
  // ---- row pointers of the lists that are grouped by query as they stand
  if (part == FL_PART_LISTS) {
    if (tid < nl) {
      const int vr = min(b_lr + S.off[1][tid], n_lr);
      A.rp_lr[l0 + tid] = vr;
      if (A.so_lr.rowptr) A.so_lr.rowptr[l0 + tid] = vr;
    }
    if (tid < nt) A.rp_tor[t0 + tid] = min(b_tor + S.off[3][tid], n_tor);
    if (last) {
      for (int i = l0 + nl + tid; i <= A.n_lig; i += FL_THREADS) {
        A.rp_lr[i] = n_lr;
        if (A.so_lr.rowptr) A.so_lr.rowptr[i] = n_lr;
      }
      if (tor)
        for (int i = t0 + nt + tid; i <= A.n_tor; i += FL_THREADS) A.rp_tor[i] = n_tor;
    }
    return;
  }
  if (part == FL_PART_LA) {
    if (tid < nl) {
      const int va = min(b_la + S.off[2][tid], n_la);
      A.rp_la[l0 + tid] = va;
      if (A.so_la.rowptr) A.so_la.rowptr[l0 + tid] = va;
    }
    if (last)
      for (int i = l0 + nl + tid; i <= A.n_lig; i += FL_THREADS) {
        A.rp_la[i] = n_la;
        if (A.so_la.rowptr) A.so_la.rowptr[i] = n_la;
      }
    return;
  }

  // ---- ligand x atom by atom (+ the near rows), ligand x receptor by residue
  if (part == FL_PART_C_LA) {
    column_view<FL_WA, true>(S.mla, S.pla, S.off[2], nl, na, b_la, n_la, a0, l0, A.n_atom, last, A.c_la, A.so_la.perm, S.wsum, A.near_rows,
                             b_near);
    return;
  }
  if (part == FL_PART_C_LR) {
    column_view<FL_WR, false>(S.mlr, S.plr, S.off[1], nl, nr, b_lr, n_lr, r0, l0, A.n_rec, last, A.c_lr, A.so_lr.perm, S.wsum, nullptr, 0);
    return;
  }

  // ---- the ligand list = bond entries + radius pairs, grouped by ll0 (c_ll), and that view grouped by ll1 (so_ll)
  const int nb = S.nbond < FL_NB ? S.nbond : FL_NB;
  int myb = 0, rank = 0;
  if (tid < nb) {
    myb = S.bl[tid];
    for (int a = 0; a < nb; ++a) rank += S.bl[a] < myb ? 1 : 0;
  }
  __syncthreads();
  if (tid < nb) S.bl[rank] = myb;           // ascending entry index (the slots were taken in arbitrary order)
  __syncthreads();
  if (tid < nb) {
    const int i = S.bl[tid];
    const int k0 = A.ll0[i] - l0;
    int k1 = A.ll1[i] - l0;
    if ((unsigned)k1 >= (unsigned)nl) k1 = k0;
    S.bk0[tid] = k0;
    S.bk1[tid] = k1;
    atomicAdd(&S.nb0[k0], 1);
    atomicAdd(&S.nb1[k1], 1);
  }
  __syncthreads();
  const int rb = b_bond + max(min(b_ll, n_ll) - Eb, 0);   // entries of the earlier samples: their bonds + their radius pairs inside n
  if (wid == 0) {
    const int k = lane;
    int cc = 0;
    if (k < nl)
      for (int q = 0; q < nl; ++q) {
        const u64 m = S.mll[q];
        if ((m >> k) & 1ull) cc += (b_ll + S.off[0][q] + __popcll(m & bits_below(k))) < n_ll ? 1 : 0;
      }
    const int len = k < nl ? S.nb0[k] + cc : 0;
    const int ex = wave_incl_scan(len, lane) - len;
    S.rs0[k] = ex;
    if (k < nl) {
      A.c_ll.rowptr[l0 + k] = rb + ex;
      int kk = 0;
      for (int q = 0; q < nl && kk < cc; ++q) {
        const u64 m = S.mll[q];
        if ((m >> k) & 1ull) {
          const int p = rb + ex + S.nb0[k] + kk;
          A.c_ll.perm[p] = b_ll + S.off[0][q] + __popcll(m & bits_below(k));
          A.c_ll.key[p] = l0 + k;
          A.c_ll.out0[p] = l0 + q;
          S.posr[q * FL_NL + k] = p;
          ++kk;
        }
      }
    }
  } else if (wid == 1) {
    const int q = lane;
    int len = 0;
    if (q < nl) len = S.nb1[q] + max(min(n_ll - (b_ll + S.off[0][q]), __popcll(S.mll[q])), 0);
    const int ex = wave_incl_scan(len, lane) - len;
    S.rs1[q] = ex;
    if (q < nl && A.so_ll.rowptr) A.so_ll.rowptr[l0 + q] = rb + ex;
  }
  if (last)
    for (int i = l0 + nl + tid; i <= A.n_lig; i += FL_THREADS) {
      A.c_ll.rowptr[i] = n_ll;
      if (A.so_ll.rowptr) A.so_ll.rowptr[i] = n_ll;
    }
  __syncthreads();
  if (tid < nb) {                           // a node's bond entries come first in its row, in entry order
    const int k = S.bk0[tid];
    int rnk = 0;
    for (int a = 0; a < tid; ++a) rnk += S.bk0[a] == k ? 1 : 0;
    const int p = rb + S.rs0[k] + rnk;
    A.c_ll.perm[p] = S.bl[tid];
    A.c_ll.key[p] = l0 + k;
    A.c_ll.out0[p] = l0 + S.bk1[tid];
    S.posb[tid] = p;
  }
  __syncthreads();
  // so_ll: a row = the entries with ll1 = q in the order of their positions in c_ll (rank counting, rows are short)
  for (int idx = tid; idx < nl * FL_NL + nb; idx += FL_THREADS) {
    int q, mypos, x, orig;
    if (idx < nl * FL_NL) {
      q = idx >> 6;
      const int j = idx & 63;
      const u64 m = S.mll[q];
      if (!((m >> j) & 1ull)) continue;
      orig = b_ll + S.off[0][q] + __popcll(m & bits_below(j));
      if (orig >= n_ll) continue;
      mypos = S.posr[q * FL_NL + j];
      x = l0 + j;
    } else {
      const int a = idx - nl * FL_NL;
      q = S.bk1[a];
      mypos = S.posb[a];
      x = l0 + S.bk0[a];
      orig = S.bl[a];
    }
    int rnk = 0;
    const u64 m = S.mll[q];
    for (u64 t = m; t != 0; t &= t - 1) {
      const int j2 = __ffsll((long long)t) - 1;
      if ((b_ll + S.off[0][q] + __popcll(m & bits_below(j2))) < n_ll) rnk += S.posr[q * FL_NL + j2] < mypos ? 1 : 0;
    }
    for (int a = 0; a < nb; ++a) rnk += (S.bk1[a] == q && S.posb[a] < mypos) ? 1 : 0;
    const int p = rb + S.rs1[q] + rnk;
    A.so_ll.perm[p] = mypos;
    A.so_ll.key[p] = l0 + q;
    A.so_ll.out0[p] = x;
    A.so_ll.out1[p] = orig;
  }
}

extern "C" int ddp_front_lists(const ddp_front_lists_t* a, int32_t* taken, void* stream) {
  if (!a || !taken) return ddp_fail(DDP_EINVAL, "ddp_front_lists: null argument");
  *taken = 0;
  const ddp_front_lists_t& A = *a;
  if (A.n_graphs < 1 || A.n_lig < 0 || A.n_rec < 0 || A.n_atom < 0 || A.n_tor < 0 || A.e_bond < 0)
    return ddp_fail(DDP_EINVAL, "ddp_front_lists: n_graphs / node totals / e_bond");
  if (!(A.r_lig > 0.f) || !(A.r_cross > 0.f) || A.ll_neighbors < 1 || A.tor_neighbors < 1 || A.cross_neighbors < 1 || A.la_neighbors < 1)
    return ddp_fail(DDP_EINVAL, "ddp_front_lists: radius / max_neighbors");
  if (A.cap_ll < A.e_bond || A.cap_lr < 0 || A.cap_la < 0 || A.cap_tor < 0) return ddp_fail(DDP_EINVAL, "ddp_front_lists: capacities");
  const bool tor = A.tor_pos != nullptr && A.n_tor > 0;
  if (!A.lig_pos || !A.rec_pos || !A.atom_pos || !A.lig_ptr || !A.rec_ptr || !A.atom_ptr || !A.scratch || !A.ll0 || !A.ll1 || !A.cnt_ll ||
      !A.lr0 || !A.lr1 || !A.cnt_lr || !A.la0 || !A.la1 || !A.cnt_la || !A.touched || !A.near_rows || !A.cnt_near || !A.rp_lr || !A.rp_la ||
      (tor && (!A.tor_ptr || !A.tor_q || !A.tor_x || !A.cnt_tor || !A.rp_tor)))
    return ddp_fail(DDP_EINVAL, "ddp_front_lists: null argument");
  const ddp_front_view_t* views[6] = {&A.c_ll, &A.c_la, &A.c_lr, &A.so_ll, &A.so_la, &A.so_lr};
  for (int i = 0; i < 6; ++i) {
    const ddp_front_view_t& v = *views[i];
    if (!v.perm || !v.key || !v.out0 || (i < 3 && !v.rowptr) || (i >= 3 && !v.out1)) return ddp_fail(DDP_EINVAL, "ddp_front_lists: null view array");
  }
  // outside the fused form's limits: nothing is launched, the caller runs the chain of the list entries
  if ((A.radius_flags & DDP_RADIUS_NEAREST) != 0) return 0;
  if (A.max_lig > DDP_FRONT_MAX_LIG || A.max_tor > DDP_FRONT_MAX_LIG || A.max_rec > DDP_FRONT_MAX_REC || A.max_atom > DDP_FRONT_MAX_ATOM ||
      A.max_bonds > DDP_FRONT_MAX_BONDS)
    return 0;
  if (A.cross_neighbors < A.max_rec || A.la_neighbors < A.max_atom) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((ddp_front_lists_kernel<false>), dim3(A.n_graphs), dim3(FL_THREADS), 0, st, A);
  hipLaunchKernelGGL((ddp_front_lists_kernel<true>), dim3(A.n_graphs, FL_PARTS), dim3(FL_THREADS), 0, st, A);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ddp_fail_hip(err, "ddp_front_lists launch");
  *taken = 1;
  return 0;
}
