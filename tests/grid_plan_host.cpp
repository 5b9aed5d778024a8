// Host build of torchmd_amd/csrc/grid_plan.h for tests/test_grid_plan_host.py: the cell grid's planner behind a plain C
// interface, compiled with the system C++ compiler.
#include "grid_plan.h"

using namespace tmd;

extern "C" {

int gp_read_stencil_knob() { return read_stencil_knob(); }  // (from the environment)

// out: nc[3], m, periodic; zreach: 49 values, row-major [ox + m][oy + m], 99 where the planner wrote nothing;
// real: inv_edge[3], origin[3].  Returns 1 when a grid was planned.
int gp_plan(int natoms, double rlist, const double *box, const double *lo, const double *hi, int stencil_knob, int *out, int *zreach,
            double *real) {
  GridPlan g;
  for (int a = 0; a < 7; ++a)
    for (int b = 0; b < 7; ++b) g.zreach[a][b] = 99;
  const bool ok = plan_grid_host(natoms, rlist, box, lo, hi, stencil_knob, g);
  if (!ok) return 0;
  for (int k = 0; k < 3; ++k) out[k] = g.nc[k], real[k] = g.inv_edge[k], real[3 + k] = g.origin[k];
  out[3] = g.m, out[4] = g.periodic;
  for (int a = 0; a < 7; ++a)
    for (int b = 0; b < 7; ++b) zreach[7 * a + b] = g.zreach[a][b];
  return 1;
}

}  // extern "C"
