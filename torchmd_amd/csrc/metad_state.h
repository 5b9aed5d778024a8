// What slot kSideMetad of a context holds, for both flavours of the bias: metad.hip (a distance of two atoms, a torsion of four)
// and metad_group.hip (CVs of groups of atoms).  The grid side (interpolant, node kernel, hills, get / set) never looks at what
// kind of CV produced s: it lives in metad.hip and serves both.  The group flavour hangs its tables on `group` and puts its
// own CV launches in the place of metad.hip's height kernel.
#pragma once

#include "engine.h"
#include "metad_math.h"

namespace tmd {

constexpr int kMetadOut = 1 + kMetadMaxCv;  // doubles per replica of the bias kernels' report: V, s_0, s_1

struct MetadState {
  int nrep = 0, natoms = 0, shared = 0;
  MetadDef def{};       // (the group flavour fills ncv, the axes and sigma: what the grid side reads)
  int64_t nodes = 0;    // per grid
  int ngrids = 0;
  DevBuf grid;          // double [ngrids][nodes][width]
  DevBuf last;          // double [R][kMetadOut]: (V, s) of the last step of the last tmdhip_md_run
  const void *mass_checked = nullptr;
  // the group flavour: its state, (a) of the deposit chain in its hands, and what frees the state
  void *group = nullptr;
  int (*group_heights)(tmdhip_ctx *ctx, const void *pos, const double *box_host, double height, double kdt, int plain, double *row,
                       hipStream_t st) = nullptr;
  void (*group_release)(MetadState *S) = nullptr;
  size_t grid_doubles() const { return (size_t)ngrids * nodes * metad_width(def); }
  const double *grid_of(int r) const { return grid.as<double>() + (shared ? 0 : (size_t)r * nodes * metad_width(def)); }
};

// what the slot's function pointers and the entry points of both flavours share
inline MetadState *metad_state_of(tmdhip_ctx *ctx) { return (MetadState *)ctx->side[kSideMetad].state; }

inline double *metad_run_energy(tmdhip_ctx *ctx) { return metad_state_of(ctx)->last.as<double>(); }

// frees a bias of either flavour and clears the slot
inline void metad_release(tmdhip_ctx *ctx) {
  MetadState *S = metad_state_of(ctx);
  if (!S) return;
  if (S->group_release) S->group_release(S);
  S->grid.release();
  S->last.release();
  delete S;
  ctx->side[kSideMetad] = SideTerm{};
}

}  // namespace tmd
