// The cell grid's host arithmetic (context.hip: plan_grid): cells per axis, the stencil half-width m with its atoms-per-cell
// rules, the cell edges and the z reach of every (x, y) stencil row — free of HIP so that it also compiles for the host alone
// (tests/grid_plan_host.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace tmd {

constexpr int kMaxCellsPerAxis = 1024;
constexpr int kMaxStencil = 3;  // the build kernel's LDS tables hold (2 * 3 + 1)^2 rows of two segments

struct GridPlan {
  int nc[3];
  int m;                     // stencil half-width in cells (1..3)
  signed char zreach[7][7];  // Grid::zreach (engine.h): index = offset + m; entries outside the stencil are left alone
  int periodic;
  double origin[3];
  double inv_edge[3];
};

// TMDHIP_STENCIL (1..3): the largest stencil half-width tried, and no coarsening of sparse grids; 0 = not set
inline int read_stencil_knob() {
  if (const char *e = std::getenv("TMDHIP_STENCIL")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= kMaxStencil) return v;
    return -1;  // set, but not a half-width: the default largest m, and still no coarsening
  }
  return 0;
}

// Largest |z offset| of stencil row (ox, oy) whose cells can hold a point within rlist of a point of the home cell: the gap
// between two cells `o` apart along an axis is (|o| - 1) edges.  -1: no cell of the row is in reach.
inline int row_zreach(int ox, int oy, int m, const double *edge, double rlist) {
  int zr = -1;
  const double gx = std::max(std::abs(ox) - 1, 0) * edge[0], gy = std::max(std::abs(oy) - 1, 0) * edge[1];
  for (int oz = 0; oz <= m; ++oz) {
    const double gz = std::max(oz - 1, 0) * edge[2];
    if (gx * gx + gy * gy + gz * gz <= rlist * rlist) zr = oz;
  }
  return zr;
}

// Grid for `box` (all zero: open boundaries, the atoms' bounds lo .. hi); false: the cell path cannot be used.
// stencil_knob: read_stencil_knob().
inline bool plan_grid_host(int natoms, double rlist, const double *box, const double *lo, const double *hi, int stencil_knob, GridPlan &g) {
  const bool periodic = !(box[0] == 0 && box[1] == 0 && box[2] == 0);
  g.periodic = periodic ? 1 : 0;
  double len[3];
  for (int k = 0; k < 3; ++k) {
    if (periodic) {
      if (!(box[k] > 0)) return false;
      len[k] = box[k];
      g.origin[k] = 0;
    } else {
      len[k] = std::max(hi[k] - lo[k], 1e-3);
      g.origin[k] = lo[k];
    }
  }
  // stencil half-width m: cell edge >= rlist/m.  m=3 (measured at C3: 29^3 cells of ~4 atoms) halves the
  // candidate volume but the build takes 345 us instead of 200: a build wave works on one cell and its
  // fixed costs (stencil set-up, staging the cell's atoms and exclusions, one candidate load per chunk)
  // are then amortised over 4 atoms instead of 14.  The kernel supports it (zreach), the planner stops at 2.
  const int mmax = stencil_knob > 0 ? stencil_knob : 2;
  for (int m = mmax; m >= 1; --m) {
    bool ok = true;
    int nc[3];
    for (int k = 0; k < 3; ++k) {
      nc[k] = (int)std::floor(len[k] / (rlist / m));
      if (nc[k] < 1) nc[k] = 1;
      if (periodic && nc[k] < 2 * m + 1) ok = false;
      if (nc[k] > kMaxCellsPerAxis) nc[k] = kMaxCellsPerAxis;
    }
    if (!ok) continue;
    // a build wave works on one cell: at gas/liquid-argon densities half-width 2 leaves ~3 atoms per cell
    // (343k cells for the 10^6-atom LJ box) and the coarser grid is faster overall (179 vs 185 us/step)
    const double per_cell = (double)natoms / ((double)nc[0] * nc[1] * nc[2]);
    if (m == 3 && per_cell < 2.0) continue;
    if (m == 2 && per_cell < 4.0 && stencil_knob == 0) {
      bool coarse_ok = true;
      for (int k = 0; k < 3; ++k) coarse_ok = coarse_ok && (!periodic || (int)std::floor(len[k] / rlist) >= 3);
      if (coarse_ok) continue;
    }
    g.m = m;
    double edge[3];
    for (int k = 0; k < 3; ++k) {
      g.nc[k] = nc[k];
      g.inv_edge[k] = nc[k] / len[k];
      edge[k] = len[k] / nc[k];
    }
    for (int ox = -m; ox <= m; ++ox)
      for (int oy = -m; oy <= m; ++oy) g.zreach[ox + m][oy + m] = (signed char)row_zreach(ox, oy, m, edge, rlist);
    return true;
  }
  return false;
}

}  // namespace tmd
