// The constrained MD step of the nonbonded engine for gfx950 (MI355X): the kernels that step a rigid water, an X-H cluster or a
// free atom in one thread, their launcher for the MD loop (md_loop.hip: launch_step) and tmdhip_set_constraints.
#include "cons_math.h"
#include "engine.h"
#include "md_step.h"
#include "vsite_math.h"

namespace tmd {

// ---- constrained MD step (tmdhip_set_constraints) ----------------------------------------------------------
// One thread owns one unit — a rigid water, an X-H cluster or an unconstrained atom — and does for every atom of it what
// md_step_atom does (f_zero, the thermostat with the noise of the atom's own row, the kicks, the drift, the displacement test,
// the cell-sorted record), with the constraints between the phases: after the second half kick the velocity constraint of the
// unit, after the drift the position constraint relative to the undrifted positions (SETTLE / SHAKE), then v += dx / dt.
// The arithmetic is double in both precisions (fp32: only the loads and stores are float).
constexpr int kConsAtom = 0, kConsWater = 1, kConsCluster = 2;

struct ConsArgs {
  const int2 *units;  // {kind, index} ordered by the unit's first atom: kConsAtom (index = atom), kConsWater, kConsCluster
  int nunits;
  const int *water;     // [W][3] O, H1, H2
  const double *wdist;  // [W][2] d_OH, d_HH
  const int *coff, *catom;
  const double *cdist;
  double tol;
  int max_iter;
  int *fail;  // host-mapped word: a unit did not converge (cons_verdict)
};

// Four-site rigid waters (tmdhip_set_vsites): the massless site of water w, or -1, and its weights in the order
// O, H1, H2 — the order of the site's parent table.  The water's thread serves the site as well (md_step_cons_vs_kernel).
struct ConsSiteArgs {
  const int *wsite;       // [W]
  const double *wweight;  // [W][3]
};

struct ConsState {
  DevBuf units, water, wdist, coff, catom, cdist;
  DevBuf wsite, wweight;  // (only with sites)
  bool has_sites = false;
  int nunits = 0;
  double tol = 1e-10;
  int max_iter = 200;
  int *fail_host = nullptr;
};

// VS (waters only): the unit also carries the massless site `site` with weights sw (parents O, H1, H2 in this order) — its force
// is folded into the parents' before anything divides by a mass, the site is placed from the parents' positions as stored, and
// it gets what every atom gets but an update: f_zero, the entry snapshot, the cell-sorted record, the displacement test;
// velocity 0.  Nothing here reads the site's mass or draws noise for it.
template <typename R, bool SECOND, bool LANGEVIN, bool FIRST, bool CHECK, int NA, int NC, bool WATER, bool VS = false>
__device__ __forceinline__ void cons_unit(const MdStepArgs<R> &s, const PairConsts<R> &c, const ConsArgs &k, const int (&at)[NA],
                                          const double (&d)[NA], size_t off, uint64_t row0, int site = -1, const double *sw = nullptr) {
#pragma clang fp contract(off)
  static_assert(!VS || (WATER && NA == 3), "a site belongs to a rigid water");
  using R4 = typename Vec<R>::T4;
  const R *vel = s.vel + off, *f = s.f + off, *pin = s.pos_in + off;
  R *pout = s.pos_out + off, *vout = s.vel + off;
  AtomIn<R> x[NA];
  AtomIn<R> xs{};  // the site: force, and with FIRST && CHECK reference point, limit, charge and slot (p, v: entry snapshot only)
  if constexpr (VS) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      xs.f[q] = f[3 * site + q];
      xs.r[q] = (FIRST && CHECK) ? s.chk.ref[3 * site + q] : R(0);
    }
    xs.q = (FIRST && CHECK) ? s.qs[site] : R(0);
    xs.h2 = (FIRST && CHECK) ? list_check_limit(s.chk, site) : R(0);
    xs.slot = (FIRST && CHECK) ? s.inv[site] : 0;
  }
#pragma unroll
  for (int j = 0; j < NA; ++j) {  // every load first (md_load_atom), the positions also without a drift (velocity constraint)
    const int i = at[j];
    x[j].m = s.mass[i];
    x[j].vc = (SECOND && LANGEVIN) ? s.vcoeff[i] : R(0);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      x[j].v[q] = vel[3 * i + q];
      x[j].f[q] = f[3 * i + q];
      x[j].p[q] = pin[3 * i + q];
      x[j].r[q] = (FIRST && CHECK) ? s.chk.ref[3 * i + q] : R(0);
    }
    x[j].q = (FIRST && CHECK) ? s.qs[i] : R(0);
    x[j].h2 = (FIRST && CHECK) ? list_check_limit(s.chk, i) : R(0);
    x[j].slot = (FIRST && CHECK) ? s.inv[i] : 0;
  }
  if constexpr (FIRST && !SECOND && CHECK) {
    if (s.snap_pos) {  // the state at the entry of the call (tmdhip_md_restore), as md_step_kernel saves it
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        const int i = at[j];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          s.snap_pos[3 * i + q] = x[j].p[q];
          s.snap_vel[3 * i + q] = x[j].v[q];
          s.snap_f[3 * i + q] = x[j].f[q];
        }
        if (s.zero && i < s.nzero) s.zero[i] = 0.0;
      }
      if constexpr (VS) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          s.snap_pos[3 * site + q] = pin[3 * site + q];
          s.snap_vel[3 * site + q] = vel[3 * site + q];
          s.snap_f[3 * site + q] = xs.f[q];
        }
        if (s.zero && site < s.nzero) s.zero[site] = 0.0;
      }
    }
  }
  if (s.f_zero) {
    R *fz = s.f_zero + off;
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) fz[3 * at[j] + q] = R(0);
    if constexpr (VS) {
#pragma unroll
      for (int q = 0; q < 3; ++q) fz[3 * site + q] = R(0);
    }
  }
  if constexpr (VS) {  // what tmdhip_vsite_spread stores in the parents' rows, rounding included
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) x[j].f[q] = vsite_share<R>(x[j].f[q], sw[j], xs.f[q]);
  }
  const double dt = (double)s.dt, hdt = (double)s.half_dt, gamma = (double)s.gamma;
  double p[NA][3], v[NA][3], a[NA][3], im[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    im[j] = 1.0 / (double)x[j].m;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      p[j][q] = x[j].p[q];
      v[j][q] = x[j].v[q];
      a[j][q] = (double)x[j].f[q] / (double)x[j].m;
    }
  }
  if (SECOND) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      if (LANGEVIN) {
        R g[3];
        normal3<R>(s.seed, s.noise_step, row0 + (uint64_t)at[j], g[0], g[1], g[2]);
#pragma unroll
        for (int q = 0; q < 3; ++q) v[j][q] += -gamma * v[j][q] * dt + (double)g[q] * (double)x[j].vc;
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) v[j][q] += hdt * a[j][q];
    }
    if constexpr (NC > 0) cons_velocities<NA, NC, WATER>(p, v, im);
  }
  if (FIRST) {
    double xn[NA][3], u[NA][3];
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        xn[j][q] = p[j][q] + (v[j][q] * dt + 0.5 * a[j][q] * dt * dt);
        u[j][q] = xn[j][q];
        v[j][q] = v[j][q] + hdt * a[j][q];
      }
    bool ok = true;
    if constexpr (WATER) ok = settle_water(p, xn, (double)x[0].m, (double)x[1].m, d[0], d[1]);
    else if constexpr (NC > 0) ok = shake_cluster<NA>(p, xn, im, d, k.tol, k.max_iter);
    if (!ok) *k.fail = 1;
    R stored[VS ? NA : 1][3];  // (VS) the parents' positions as rounded for storage
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int i = at[j];
      R pr[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (NC > 0) v[j][q] += (xn[j][q] - u[j][q]) / dt;
        pr[q] = (R)xn[j][q];
        pout[3 * i + q] = pr[q];
        if constexpr (VS) stored[j][q] = pr[q];
      }
      if (CHECK) {
        R4 sv;
        sv.x = pr[0];
        sv.y = pr[1];
        sv.z = pr[2];
        sv.w = x[j].q;
        s.sorted[x[j].slot] = sv;
        extent_note<R>(s.chk.ext, pr[0], pr[1], pr[2]);
        list_check_point<R>(s.chk, c, pr[0] - x[j].r[0], pr[1] - x[j].r[1], pr[2] - x[j].r[2], x[j].h2);
      }
    }
    if constexpr (VS) {  // the site, from the stored parents: tmdhip_vsite_construct's expression
      R pr[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        pr[q] = vsite_coord<R>(sw[0], sw[1], sw[2], stored[0][q], stored[1][q], stored[2][q], true);
        pout[3 * site + q] = pr[q];
      }
      if (CHECK) {
        R4 sv;
        sv.x = pr[0];
        sv.y = pr[1];
        sv.z = pr[2];
        sv.w = xs.q;
        s.sorted[xs.slot] = sv;
        extent_note<R>(s.chk.ext, pr[0], pr[1], pr[2]);
        list_check_point<R>(s.chk, c, pr[0] - xs.r[0], pr[1] - xs.r[1], pr[2] - xs.r[2], xs.h2);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NA; ++j)
#pragma unroll
    for (int q = 0; q < 3; ++q) vout[3 * at[j] + q] = (R)v[j][q];
  if constexpr (VS) {
#pragma unroll
    for (int q = 0; q < 3; ++q) vout[3 * site + q] = R(0);
  }
}

template <typename R, bool SECOND, bool LANGEVIN, bool FIRST, bool CHECK, int NA>
__device__ __forceinline__ void cons_cluster(const MdStepArgs<R> &s, const PairConsts<R> &c, const ConsArgs &k, int s0, size_t off,
                                             uint64_t row0) {
  int at[NA];
  double d[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    at[j] = k.catom[s0 + j];
    d[j] = k.cdist[s0 + j];
  }
  cons_unit<R, SECOND, LANGEVIN, FIRST, CHECK, NA, NA - 1, false>(s, c, k, at, d, off, row0);
}

// Without CHECK (all-pairs contexts) blockIdx.y is the replica, as in md_step_kernel.
template <typename R, bool SECOND, bool LANGEVIN, bool FIRST, bool CHECK>
__global__ __launch_bounds__(256) void md_step_cons_kernel(MdStepArgs<R> s, PairConsts<R> c, ConsArgs k) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (CHECK && u == 0) list_check_clear(s.chk.flags, s.chk.parity);
  if (u >= k.nunits) return;
  const size_t off = CHECK ? 0 : (size_t)blockIdx.y * 3 * s.n;
  const uint64_t row0 = s.row0 + (CHECK ? 0 : (uint64_t)blockIdx.y * (uint64_t)s.n);
  const int2 e = k.units[u];
  if (e.x == kConsWater) {
    const int at[3] = {k.water[3 * e.y], k.water[3 * e.y + 1], k.water[3 * e.y + 2]};
    const double d[3] = {k.wdist[2 * e.y], k.wdist[2 * e.y + 1], 0.0};
    cons_unit<R, SECOND, LANGEVIN, FIRST, CHECK, 3, 3, true>(s, c, k, at, d, off, row0);
  } else if (e.x == kConsCluster) {
    const int s0 = k.coff[e.y], na = k.coff[e.y + 1] - s0;
    switch (na) {
      case 2: cons_cluster<R, SECOND, LANGEVIN, FIRST, CHECK, 2>(s, c, k, s0, off, row0); break;
      case 3: cons_cluster<R, SECOND, LANGEVIN, FIRST, CHECK, 3>(s, c, k, s0, off, row0); break;
      case 4: cons_cluster<R, SECOND, LANGEVIN, FIRST, CHECK, 4>(s, c, k, s0, off, row0); break;
      default: cons_cluster<R, SECOND, LANGEVIN, FIRST, CHECK, 5>(s, c, k, s0, off, row0); break;
    }
  } else {
    const int at[1] = {e.y};
    const double d[1] = {0.0};
    cons_unit<R, SECOND, LANGEVIN, FIRST, CHECK, 1, 0, false>(s, c, k, at, d, off, row0);
  }
}

// The same for a context with virtual sites: a water with a site is stepped together with it.
template <typename R, bool SECOND, bool LANGEVIN, bool FIRST, bool CHECK>
__global__ __launch_bounds__(256) void md_step_cons_vs_kernel(MdStepArgs<R> s, PairConsts<R> c, ConsArgs k, ConsSiteArgs vs) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (CHECK && u == 0) list_check_clear(s.chk.flags, s.chk.parity);
  if (u >= k.nunits) return;
  const size_t off = CHECK ? 0 : (size_t)blockIdx.y * 3 * s.n;
  const uint64_t row0 = s.row0 + (CHECK ? 0 : (uint64_t)blockIdx.y * (uint64_t)s.n);
  const int2 e = k.units[u];
  if (e.x == kConsWater) {
    const int at[3] = {k.water[3 * e.y], k.water[3 * e.y + 1], k.water[3 * e.y + 2]};
    const double d[3] = {k.wdist[2 * e.y], k.wdist[2 * e.y + 1], 0.0};
    const int site = vs.wsite[e.y];
    if (site >= 0) {
      const double sw[3] = {vs.wweight[3 * e.y], vs.wweight[3 * e.y + 1], vs.wweight[3 * e.y + 2]};
      cons_unit<R, SECOND, LANGEVIN, FIRST, CHECK, 3, 3, true, true>(s, c, k, at, d, off, row0, site, sw);
    } else {
      cons_unit<R, SECOND, LANGEVIN, FIRST, CHECK, 3, 3, true>(s, c, k, at, d, off, row0);
    }
  } else if (e.x == kConsCluster) {
    const int s0 = k.coff[e.y], na = k.coff[e.y + 1] - s0;
    switch (na) {
      case 2: cons_cluster<R, SECOND, LANGEVIN, FIRST, CHECK, 2>(s, c, k, s0, off, row0); break;
      case 3: cons_cluster<R, SECOND, LANGEVIN, FIRST, CHECK, 3>(s, c, k, s0, off, row0); break;
      case 4: cons_cluster<R, SECOND, LANGEVIN, FIRST, CHECK, 4>(s, c, k, s0, off, row0); break;
      default: cons_cluster<R, SECOND, LANGEVIN, FIRST, CHECK, 5>(s, c, k, s0, off, row0); break;
    }
  } else {
    const int at[1] = {e.y};
    const double d[1] = {0.0};
    cons_unit<R, SECOND, LANGEVIN, FIRST, CHECK, 1, 0, false>(s, c, k, at, d, off, row0);
  }
}

static ConsArgs cons_args(const tmdhip_ctx *ctx) {
  const ConsState *S = (const ConsState *)ctx->cons;
  ConsArgs k;
  k.units = S->units.as<int2>();
  k.nunits = S->nunits;
  k.water = S->water.as<int>();
  k.wdist = S->wdist.as<double>();
  k.coff = S->coff.as<int>();
  k.catom = S->catom.as<int>();
  k.cdist = S->cdist.as<double>();
  k.tol = S->tol;
  k.max_iter = S->max_iter;
  k.fail = S->fail_host;
  return k;
}

void cons_release(tmdhip_ctx *ctx) {
  ConsState *S = (ConsState *)ctx->cons;
  if (!S) return;
  for (DevBuf *b : {&S->units, &S->water, &S->wdist, &S->coff, &S->catom, &S->cdist, &S->wsite, &S->wweight}) b->release();
  if (S->fail_host) (void)hipHostFree(S->fail_host);
  delete S;
  ctx->cons = nullptr;
}

int cons_verdict(tmdhip_ctx *ctx) {
  ConsState *S = (ConsState *)ctx->cons;
  if (!S || !S->fail_host || !*(volatile int *)S->fail_host) return 0;
  *(volatile int *)S->fail_host = 0;
  return fail("constrained MD step: a SHAKE cluster did not converge within max_iter sweeps, or a water was too distorted for "
              "SETTLE; the trajectory since the previous call is invalid");
}

bool cons_has_sites(const tmdhip_ctx *ctx) { return ctx->cons && ((const ConsState *)ctx->cons)->has_sites; }

// the constrained integrator kernel of one phase of md_run (for_md_phase: the five that exist), with the site variant when the
// context's waters carry virtual sites
template <typename R>
void launch_cons_step(const tmdhip_ctx *ctx, const MdStepArgs<R> &a, const PairConsts<R> &c, bool second, bool langevin, bool first,
                      bool check, int nrep, hipStream_t st) {
  const ConsArgs k = cons_args(ctx);
  const dim3 grid((k.nunits + 255) / 256, check ? 1 : nrep), block(256);
  const ConsState *S = (const ConsState *)ctx->cons;
  const ConsSiteArgs vs{S->wsite.as<int>(), S->wweight.as<double>()};
  for_md_phase(second, langevin, first, [&](auto s, auto l, auto f) {
    constexpr bool SECOND = decltype(s)::value, LANGEVIN = decltype(l)::value, FIRST = decltype(f)::value;
    if (S->has_sites) {
      if (check)
        hipLaunchKernelGGL((md_step_cons_vs_kernel<R, SECOND, LANGEVIN, FIRST, true>), grid, block, 0, st, a, c, k, vs);
      else
        hipLaunchKernelGGL((md_step_cons_vs_kernel<R, SECOND, LANGEVIN, FIRST, false>), grid, block, 0, st, a, c, k, vs);
    } else if (check) {
      hipLaunchKernelGGL((md_step_cons_kernel<R, SECOND, LANGEVIN, FIRST, true>), grid, block, 0, st, a, c, k);
    } else {
      hipLaunchKernelGGL((md_step_cons_kernel<R, SECOND, LANGEVIN, FIRST, false>), grid, block, 0, st, a, c, k);
    }
  });
}
template void launch_cons_step<float>(const tmdhip_ctx *, const MdStepArgs<float> &, const PairConsts<float> &, bool, bool, bool, bool, int,
                                      hipStream_t);
template void launch_cons_step<double>(const tmdhip_ctx *, const MdStepArgs<double> &, const PairConsts<double> &, bool, bool, bool, bool,
                                       int, hipStream_t);

}  // namespace tmd

using namespace tmd;

extern "C" {

int tmdhip_set_constraints(tmdhip_ctx *ctx, const tmdhip_constraint_desc *desc) {
  if (!ctx || !desc) return fail("tmdhip_set_constraints: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_constraint_desc))
    return fail("tmdhip_set_constraints: tmdhip_constraint_desc size mismatch (ABI)");
  cons_release(ctx);
  if (!desc->enable || (desc->nwaters <= 0 && desc->nclusters <= 0)) return 0;
  const int n = ctx->d.natoms, nw = std::max(desc->nwaters, 0), nc = std::max(desc->nclusters, 0);
  if ((nw && (!desc->water_host || !desc->water_dist_host)) ||
      (nc && (!desc->cluster_offsets_host || !desc->cluster_atoms_host || !desc->cluster_dist_host)))
    return fail("tmdhip_set_constraints: null array");
  if (!(desc->tolerance > 0) || desc->max_iter < 1) return fail("tmdhip_set_constraints: tolerance must be > 0 and max_iter >= 1");
  // units ordered by their first atom: neighbouring threads touch neighbouring atoms
  std::vector<int> owner(n, -1);
  std::vector<std::pair<int, int2>> units;
  auto take = [&](int i, int tag) {
    if (i < 0 || i >= n) return fail("tmdhip_set_constraints: atom index out of range");
    if (owner[i] >= 0) return fail("tmdhip_set_constraints: atom " + std::to_string(i) + " is in two constraint units");
    owner[i] = tag;
    return 0;
  };
  for (int w = 0; w < nw; ++w) {
    const int32_t *a = desc->water_host + 3 * w;
    const double doh = desc->water_dist_host[2 * w], dhh = desc->water_dist_host[2 * w + 1];
    if (!(doh > 0) || !(dhh > 0) || !(dhh < 2 * doh)) return fail("tmdhip_set_constraints: water distances must satisfy 0 < d_HH < 2 d_OH");
    for (int j = 0; j < 3; ++j) TMD_TRY(take(a[j], 1));
    units.push_back({std::min({a[0], a[1], a[2]}), make_int2(kConsWater, w)});
  }
  const int32_t *off = desc->cluster_offsets_host;
  if (nc && off[0] != 0) return fail("tmdhip_set_constraints: cluster offsets must start at 0");
  for (int q = 0; q < nc; ++q) {
    const int na = off[q + 1] - off[q];
    if (na < 2 || na > 5) return fail("tmdhip_set_constraints: a cluster has 2 .. 5 atoms (1 .. 4 constraints)");
    int lo = n;
    for (int j = off[q]; j < off[q + 1]; ++j) {
      TMD_TRY(take(desc->cluster_atoms_host[j], 2));
      if (j > off[q] && !(desc->cluster_dist_host[j] > 0)) return fail("tmdhip_set_constraints: bond lengths must be positive");
      lo = std::min(lo, (int)desc->cluster_atoms_host[j]);
    }
    units.push_back({lo, make_int2(kConsCluster, q)});
  }
  // virtual sites: each belongs to the water whose O, H1, H2 are its parents (in this order), and is no unit of its own
  const VsiteState *V = (const VsiteState *)ctx->vsites;
  std::vector<int32_t> wsite;
  std::vector<double> wweight;
  if (V) {
    std::vector<int> water_of(n, -1);
    for (int w = 0; w < nw; ++w) water_of[desc->water_host[3 * w]] = w;
    wsite.assign(nw, -1);
    wweight.assign(3 * (size_t)nw, 0.0);
    for (int s = 0; s < V->nsites; ++s) {
      const int32_t *pa = V->parent_h.data() + 3 * (size_t)s;
      const int w = (pa[0] >= 0 && pa[0] < n) ? water_of[pa[0]] : -1;
      if (w < 0 || wsite[w] >= 0 || pa[1] != desc->water_host[3 * w + 1] || pa[2] != desc->water_host[3 * w + 2])
        return fail("tmdhip_set_constraints: the parents of virtual site " + std::to_string(V->site_h[s]) +
                    " are not the O, H1, H2 (in this order) of one rigid water");
      TMD_TRY(take(V->site_h[s], 3));
      wsite[w] = V->site_h[s];
      for (int k = 0; k < 3; ++k) wweight[3 * (size_t)w + k] = V->weight_h[3 * (size_t)s + k];
    }
  }
  for (int i = 0; i < n; ++i)
    if (owner[i] < 0) units.push_back({i, make_int2(kConsAtom, i)});
  std::sort(units.begin(), units.end(), [](const std::pair<int, int2> &x, const std::pair<int, int2> &y) { return x.first < y.first; });
  std::vector<int2> u(units.size());
  for (size_t j = 0; j < units.size(); ++j) u[j] = units[j].second;
  auto *S = new ConsState();
  ctx->cons = S;
  auto up = [&](DevBuf &b, const void *src, size_t bytes) {
    TMD_TRY(b.ensure(std::max<size_t>(bytes, 16)));
    if (bytes) TMD_HIP(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  const int ncat = nc ? off[nc] : 0;
  int rc = up(S->units, u.data(), sizeof(int2) * u.size());
  if (!rc) rc = up(S->water, desc->water_host, sizeof(int32_t) * 3 * nw);
  if (!rc) rc = up(S->wdist, desc->water_dist_host, sizeof(double) * 2 * nw);
  if (!rc) rc = up(S->coff, desc->cluster_offsets_host, nc ? sizeof(int32_t) * (nc + 1) : 0);
  if (!rc) rc = up(S->catom, desc->cluster_atoms_host, sizeof(int32_t) * ncat);
  if (!rc) rc = up(S->cdist, desc->cluster_dist_host, sizeof(double) * ncat);
  if (!rc && V && nw) {
    rc = up(S->wsite, wsite.data(), sizeof(int32_t) * nw);
    if (!rc) rc = up(S->wweight, wweight.data(), sizeof(double) * 3 * nw);
    S->has_sites = !rc;
  }
  if (!rc && hipHostMalloc((void **)&S->fail_host, 64, hipHostMallocMapped) != hipSuccess) rc = fail("tmdhip_set_constraints: hipHostMalloc failed");
  if (rc) {
    cons_release(ctx);
    return rc;
  }
  *(volatile int *)S->fail_host = 0;
  S->nunits = (int)u.size();
  S->tol = desc->tolerance;
  S->max_iter = desc->max_iter;
  return 0;
}

}  // extern "C"
