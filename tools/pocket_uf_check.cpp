// pocket_uf_check.cpp - the union-find helpers of ddp_pocket_label (csrc/ddp_pockets_uf.h) on the host, for the host sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread -I diffdock_pocket_amd/csrc tools/pocket_uf_check.cpp -o pocket_uf_check
//   ./pocket_uf_check
//
// Runs init / union over the +x, +y, +z neighbours / flatten as the three kernels do - once in index order, once in reverse order and
// once from 8 threads over interleaved points - on the masks of tests/test_gpu_pockets.py and compares every label with a flood fill.
// Exit status 0 and "ok" when every case agrees.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "ddp_pockets_uf.h"

struct Grid {
  int nx, ny, nz;
  std::vector<int32_t> mask;
  int n() const { return nx * ny * nz; }
};

static std::vector<int32_t> flood(const Grid& g) {
  std::vector<int32_t> lab(g.n(), -1), stack;
  for (int s = 0; s < g.n(); ++s) {
    if (!g.mask[s] || lab[s] >= 0) continue;
    lab[s] = s;      // seeds come in ascending order: the seed is the component's smallest index
    stack.assign(1, s);
    while (!stack.empty()) {
      const int p = stack.back();
      stack.pop_back();
      const int k = p % g.nz, j = (p / g.nz) % g.ny, i = p / (g.nz * g.ny);
      const int nb[6] = {k + 1 < g.nz ? p + 1 : -1, k > 0 ? p - 1 : -1, j + 1 < g.ny ? p + g.nz : -1, j > 0 ? p - g.nz : -1,
                         i + 1 < g.nx ? p + g.ny * g.nz : -1, i > 0 ? p - g.ny * g.nz : -1};
      for (int q : nb)
        if (q >= 0 && g.mask[q] && lab[q] < 0) {
          lab[q] = s;
          stack.push_back(q);
        }
    }
  }
  return lab;
}

static void union_point(const Grid& g, int32_t* parent, int p) {
  if (!g.mask[p]) return;
  const int k = p % g.nz, j = (p / g.nz) % g.ny, i = p / (g.nz * g.ny);
  if (k + 1 < g.nz && g.mask[p + 1]) uf_union(parent, p, p + 1);
  if (j + 1 < g.ny && g.mask[p + g.nz]) uf_union(parent, p, p + g.nz);
  if (i + 1 < g.nx && g.mask[p + g.ny * g.nz]) uf_union(parent, p, p + g.ny * g.nz);
}

static void flatten_point(int32_t* parent, int p) {
  const int32_t q = uf_load(parent + p);
  if (q < 0 || q == p) return;
  const int32_t r = uf_find(parent, q);
  if (r != q) __atomic_store_n(parent + p, r, __ATOMIC_RELAXED);
}

// mode 0: ascending, 1: descending, 2: 8 threads, thread t takes the points p % 8 == t
static std::vector<int32_t> label(const Grid& g, int mode) {
  const int n = g.n();
  std::vector<int32_t> parent(n);
  for (int p = 0; p < n; ++p) parent[p] = g.mask[p] ? p : -1;
  auto sweep = [&](const std::function<void(int)>& f) {
    if (mode == 0) {
      for (int p = 0; p < n; ++p) f(p);
    } else if (mode == 1) {
      for (int p = n - 1; p >= 0; --p) f(p);
    } else {
      std::vector<std::thread> th;
      for (int t = 0; t < 8; ++t)
        th.emplace_back([&, t] {
          for (int p = t; p < n; p += 8) f(p);
        });
      for (auto& x : th) x.join();
    }
  };
  sweep([&](int p) { union_point(g, parent.data(), p); });
  sweep([&](int p) { flatten_point(parent.data(), p); });
  return parent;
}

static int failures = 0;

static void check(const std::string& name, const Grid& g) {
  const std::vector<int32_t> want = flood(g);
  for (int mode = 0; mode < 3; ++mode)
    for (int rep = 0; rep < (mode == 2 ? 4 : 1); ++rep) {
      const std::vector<int32_t> got = label(g, mode);
      if (got != want) {
        std::printf("MISMATCH %s mode %d\n", name.c_str(), mode);
        ++failures;
      }
    }
}

static Grid make(int nx, int ny, int nz, int fill) { return Grid{nx, ny, nz, std::vector<int32_t>((size_t)nx * ny * nz, fill)}; }

int main() {
  {   // one-voxel-wide serpentine through 32 x 32 x 4: walls between the rows and the layers, one gap at alternating ends
    Grid g = make(32, 32, 4, 0);
    for (int k = 0; k < 4; k += 2)
      for (int i = 0; i < 32; ++i)
        for (int j = 0; j < 32; ++j) {
          const bool row = i % 2 == 0, gap = i % 2 == 1 && j == ((i / 2) % 2 == 0 ? 31 : 0);
          if (row || gap) g.mask[(i * 32 + j) * 4 + k] = 1;
        }
    g.mask[(30 * 32 + 31) * 4 + 1] = 1;   // the link between the two layers
    check("serpentine", g);
  }
  {
    Grid g = make(6, 6, 6, 0);   // two blobs that touch across an edge only, and a third across a corner only
    auto at = [&](int i, int j, int k) -> int32_t& { return g.mask[(i * 6 + j) * 6 + k]; };
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j)
        for (int k = 0; k < 2; ++k) at(i, j, k) = at(i + 2, j + 2, k) = at(i + 4, j + 4, k + 2) = 1;
    check("edge and corner", g);
  }
  {
    Grid g = make(7, 9, 11, 0);
    for (int p = 0; p < g.n(); ++p) {
      const int k = p % 11, j = (p / 11) % 9, i = p / 99;
      g.mask[p] = (i + j + k) % 2;
    }
    check("checkerboard", g);
  }
  check("empty", make(5, 7, 9, 0));
  check("full", make(33, 65, 17, 1));
  check("line", make(1, 1, 70, 1));
  std::mt19937 rng(0);
  for (int pct : {10, 31, 60})
    for (int big = 0; big < 2; ++big) {
      Grid g = big ? make(33, 65, 17, 0) : make(5, 7, 9, 0);
      for (auto& m : g.mask) m = (int)(rng() % 100) < pct ? (int)(rng() % 8) + 1 : 0;
      check("random " + std::to_string(pct) + (big ? " big" : " small"), g);
    }
  std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
