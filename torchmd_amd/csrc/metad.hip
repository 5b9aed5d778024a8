// Well-tempered metadynamics on one or two collective variables, for gfx950 (tmdhip_set_metadynamics, tmdhip_metad_apply,
// tmdhip_metad_deposit, tmdhip_metad_energy, tmdhip_metad_get_grid / tmdhip_metad_set_grid; the arithmetic: metad_math.h).
//
// The bias kernel: ONE WAVE PER REPLICA (blockIdx.x), ONE THREAD PER DISTINCT CV ATOM (at most 8 lanes work).  Every working
// lane evaluates the CVs and the Hermite interpolant of its replica's grid for itself (the same few loads, no exchange between
// lanes), sums its atom's contributions from both CVs in CV order and is the only writer of its atom: no atomics, and two runs
// give the same bits.  Whatever pointer is not null is served, as in restraint.hip:
//   impulse   vel only           v = R((double)v + kick F_b / m)            between two launches of tmdhip_md_run
//   finish    vel, forces, out   ... and f = R((double)f + F_b), (V, s)     after the last step of a call
//   evaluate  forces and / or out                                           tmdhip_metad_apply
// Arithmetic in double from positions of either dtype, one rounding on each store; rows of other atoms are never read or
// written.  The boxes, and where each replica's positions live, travel as kernel arguments, kSideChunk replicas per launch.
// Latency-bound: positions -> 4 or 16 nodes of 16 or 32 bytes -> one store per component.
//
// The deposit chain, two launches and no host synchronisation: (a) one wave per replica evaluates s0 and V(s0) on the grid AS
// IT IS and writes (s0..., w) into the caller's row of the hills log; (b) one thread per grid node, blockIdx.y = grid, reads
// the hills of its grid (one, or with shared walkers all R in replica order) and does one read-modify-write of its node: one
// writer per node, no floating-point atomics.  (b) is exp-bound (R exponentials per node behind a 16 / 32 byte load and
// store, both one vector access per lane; consecutive lanes take consecutive nodes).
//
// A bias on CVs of groups of atoms (tmdhip_set_metadynamics_groups, metad_group.hip) lives in the same slot and the same
// MetadState (metad_state.h): the grid, (b), the energy row, get / set and release here serve it unchanged; in the place of
// (a) it runs its own gather and heights (MetadState::group_heights), which leave the same log rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.h"
#include "metad_math.h"
#include "metad_state.h"

using namespace tmd;

namespace {

constexpr int kNodeThreads = 256;   // the node kernel's block
constexpr int kOut = kMetadOut;  // doubles per replica of the bias kernel's report: V, s_0, s_1

// the positions of the CVs' atoms, in each CV's order, as doubles
template <typename R>
__device__ __forceinline__ void load_cv_atoms(const MetadDef &D, const R *p, double (&x)[kMetadMaxCv][4][3]) {
  for (int c = 0; c < kMetadMaxCv; ++c)
    for (int a = 0; a < 4; ++a) {
      const int i = c < D.ncv ? D.atom[c][a] : -1;
      for (int k = 0; k < 3; ++k) x[c][a][k] = i >= 0 ? (double)p[3 * (size_t)i + k] : 0.0;
    }
}

// forces / vel: the rows of the launch's first replica (blockIdx.x counts from it); rep0: that replica's index
template <typename R>
__global__ __launch_bounds__(64) void metad_bias_kernel(MetadDef D, const double *__restrict__ grid, size_t grid_stride, int natoms,
                                                        R *__restrict__ forces, R *__restrict__ vel, const R *__restrict__ mass,
                                                        double kick, double *__restrict__ out, SideChunk B, int rep0) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  if (t >= D.nrows) return;
  const int r = rep0 + blockIdx.x;
  const size_t base = (size_t)blockIdx.x * natoms * 3;
  const double box[3] = {B.box[blockIdx.x][0], B.box[blockIdx.x][1], B.box[blockIdx.x][2]};
  double x[kMetadMaxCv][4][3], g[kMetadMaxCv][4][3], s[kMetadMaxCv] = {0.0, 0.0}, dV[kMetadMaxCv], f[3];
  load_cv_atoms<R>(D, (const R *)B.pos[blockIdx.x], x);
  metad_cvs(D, x, box, s, g);
  const double V = metad_interp(D, grid + (size_t)r * grid_stride, s, dV);
  metad_row_force(D, t, dV, g, f);
  const int a = D.row_atom[t];
  side_store(forces, vel, base + 3 * (size_t)a, mass, a, kick, f);
  if (out && t == 0) {
    out[(size_t)r * kOut] = V;
    for (int c = 0; c < kMetadMaxCv; ++c) out[(size_t)r * kOut + 1 + c] = s[c];
  }
}

// (a) of the deposit chain: one wave per replica (lane 0 works), row[r] = (s0..., w) with V(s0) read from the grid as it is
template <typename R>
__global__ __launch_bounds__(64) void metad_height_kernel(MetadDef D, const double *__restrict__ grid, size_t grid_stride,
                                                          double height, double kdt, int plain, double *__restrict__ row, SideChunk B,
                                                          int rep0) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  const int r = rep0 + blockIdx.x;
  const double box[3] = {B.box[blockIdx.x][0], B.box[blockIdx.x][1], B.box[blockIdx.x][2]};
  double x[kMetadMaxCv][4][3], g[kMetadMaxCv][4][3], s[kMetadMaxCv] = {0.0, 0.0}, dV[kMetadMaxCv];
  load_cv_atoms<R>(D, (const R *)B.pos[blockIdx.x], x);
  metad_cvs(D, x, box, s, g);
  const double V = metad_interp(D, grid + (size_t)r * grid_stride, s, dV);
  double *o = row + (size_t)r * (D.ncv + 1);
  for (int c = 0; c < D.ncv; ++c) o[c] = s[c];
  o[D.ncv] = metad_height(height, V, kdt, plain);
}

// (b): one thread per node, blockIdx.y = grid; the grid's hills are rows hill0 .. hill0 + nhills - 1 of `row`, added in order
template <int W>
__global__ __launch_bounds__(kNodeThreads) void metad_node_kernel(MetadDef D, double *__restrict__ grid, int64_t nodes,
                                                                  const double *__restrict__ row, int shared, int nrep) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)blockIdx.x * kNodeThreads + threadIdx.x;
  if (n >= nodes) return;
  int k[kMetadMaxCv];
  if (W == 2) {
    k[0] = (int)n;
    k[1] = 0;
  } else {
    k[0] = (int)(n / D.axis[1].nodes);
    k[1] = (int)(n % D.axis[1].nodes);
  }
  typedef double __attribute__((ext_vector_type(W))) node_t;  // 16 or 32 bytes: one vector access per lane
  node_t *cell = (node_t *)grid + ((size_t)blockIdx.y * nodes + n);
  node_t v = *cell;
  const int hill0 = shared ? 0 : (int)blockIdx.y, nhills = shared ? nrep : 1;
  for (int q = 0; q < nhills; ++q) {
    const double *hl = row + (size_t)(hill0 + q) * (D.ncv + 1);
    double add[4];
    metad_gauss(D, k, hl, hl[D.ncv], add);
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = v[c] + add[c];
  }
  *cell = v;
}

// replicas rep0 .. rep0 + nrep - 1; forces / vel point at the rows of replica rep0, box_host at its box; the positions are
// [nrep][N][3] at `pos`, or, with `pos_each`, one array per replica; `out` (double [R][kOut], indexed by the replica's number)
template <typename R>
int launch(MetadState *S, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces,
           void *vel, const void *mass, double kick, double *out, hipStream_t st) {
  const size_t stride = (size_t)S->natoms * 3;
  const size_t gstride = S->shared ? 0 : (size_t)S->nodes * metad_width(S->def);
  for (int c0 = 0; c0 < nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, nrep - c0);
    const SideChunk B = side_chunk(nr, c0, pos, pos_each, box_host, stride * sizeof(R));
    hipLaunchKernelGGL(metad_bias_kernel<R>, dim3((unsigned)nr), dim3(64), 0, st, S->def, S->grid.as<double>(), gstride, S->natoms,
                       forces ? (R *)forces + c0 * stride : nullptr, vel ? (R *)vel + c0 * stride : nullptr, (const R *)mass, kick, out,
                       B, rep0 + c0);
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

static_assert(kSideWidth[kSideMetad] == kOut, "the bias kernel reports kOut doubles per replica");
MetadState *state_of(tmdhip_ctx *ctx) { return metad_state_of(ctx); }

int launch_any(tmdhip_ctx *ctx, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces,
               void *vel, const void *mass, double kick, double *out, hipStream_t st) {
  MetadState *S = state_of(ctx);
  return ctx->d.dtype == TMDHIP_F32 ? launch<float>(S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st)
                                    : launch<double>(S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st);
}

// (the group flavour, metad_group.hip, has produced the log rows already: `heights` = false)
template <typename R>
int launch_deposit(MetadState *S, const void *pos, const double *box_host, double height, double kdt, int plain, double *row,
                   hipStream_t st, bool heights = true) {
  const size_t stride = (size_t)S->natoms * 3;
  const size_t gstride = S->shared ? 0 : (size_t)S->nodes * metad_width(S->def);
  for (int c0 = 0; heights && c0 < S->nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, S->nrep - c0);
    const SideChunk B = side_chunk(nr, c0, pos, nullptr, box_host, stride * sizeof(R));
    hipLaunchKernelGGL(metad_height_kernel<R>, dim3((unsigned)nr), dim3(64), 0, st, S->def, S->grid.as<double>(), gstride, height, kdt,
                       plain, row, B, c0);
  }
  const dim3 blocks((unsigned)((S->nodes + kNodeThreads - 1) / kNodeThreads), (unsigned)S->ngrids);
  if (S->def.ncv == 1)
    hipLaunchKernelGGL(metad_node_kernel<2>, blocks, dim3(kNodeThreads), 0, st, S->def, S->grid.as<double>(), S->nodes, row, S->shared, S->nrep);
  else
    hipLaunchKernelGGL(metad_node_kernel<4>, blocks, dim3(kNodeThreads), 0, st, S->def, S->grid.as<double>(), S->nodes, row, S->shared, S->nrep);
  TMD_HIP(hipGetLastError());
  return 0;
}

// a CV atom without mass has no acceleration: refused where masses are first seen (one read-back per mass array)
int check_masses(tmdhip_ctx *ctx, const char *, const double *, const void *mass_dev, hipStream_t st) {
  MetadState *S = state_of(ctx);
  if (!mass_dev || S->mass_checked == mass_dev) return 0;
  std::vector<char> host((size_t)ctx->real_size * S->natoms);
  TMD_HIP(hipMemcpyAsync(host.data(), mass_dev, host.size(), hipMemcpyDeviceToHost, st));
  TMD_HIP(hipStreamSynchronize(st));
  for (int t = 0; t < S->def.nrows; ++t) {
    const int32_t a = S->def.row_atom[t];
    const double m = ctx->d.dtype == TMDHIP_F32 ? (double)((const float *)host.data())[a] : ((const double *)host.data())[a];
    if (!(m > 0.0)) return fail("metadynamics: atom " + std::to_string(a) + " belongs to a CV and has no mass");
  }
  S->mass_checked = mass_dev;
  return 0;
}

void release(tmdhip_ctx *ctx) { metad_release(ctx); }

}  // namespace

extern "C" {

int tmdhip_set_metadynamics(tmdhip_ctx *ctx, const tmdhip_metad_desc *desc) {
  if (!ctx || !desc) return fail("tmdhip_set_metadynamics: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_metad_desc)) return fail("tmdhip_set_metadynamics: tmdhip_metad_desc size mismatch (ABI)");
  if (!desc->enable) {
    TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the grid may still be in flight)
    release(ctx);
    return 0;
  }
  const int n = ctx->d.natoms, nrep = (int)ctx->rep.size();
  if (desc->nreplicas != nrep) return fail("tmdhip_set_metadynamics: nreplicas must be the context's");
  if (ctx->nactive < n) return fail("tmdhip_set_metadynamics: not for a context with passive atoms (a brick of the domain decomposition)");
  const std::string why = metad_validate(n, desc->ncv, desc->kind, &desc->atoms[0][0], desc->bins, desc->grid_min, desc->grid_max, desc->sigma);
  if (!why.empty()) return fail("tmdhip_set_metadynamics: " + why);
  const MetadDef D = metad_define(desc->ncv, desc->kind, &desc->atoms[0][0], desc->bins, desc->grid_min, desc->grid_max, desc->sigma);
  if (ctx->vsites) {
    const VsiteState *V = (const VsiteState *)ctx->vsites;
    for (int t = 0; t < D.nrows; ++t)
      if (std::find(V->site_h.begin(), V->site_h.end(), D.row_atom[t]) != V->site_h.end())
        return fail("tmdhip_set_metadynamics: atom " + std::to_string(D.row_atom[t]) + " is a virtual site (use its parents)");
  }
  TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the old grid may still be in flight)
  release(ctx);
  MetadState *S = new MetadState;
  ctx->side[kSideMetad] = SideTerm{S, "metadynamics needs", launch_any, check_masses, metad_run_energy, metad_release};
  S->nrep = nrep;
  S->natoms = n;
  S->shared = desc->shared ? 1 : 0;
  S->def = D;
  S->nodes = metad_nodes(D);
  S->ngrids = S->shared ? 1 : nrep;
  int rc = S->grid.ensure(sizeof(double) * S->grid_doubles());
  if (rc == 0) rc = S->last.ensure(sizeof(double) * kOut * (size_t)nrep);
  if (rc == 0 && (hipMemset(S->grid.p, 0, S->grid.bytes) != hipSuccess || hipMemset(S->last.p, 0, S->last.bytes) != hipSuccess))
    rc = fail("tmdhip_set_metadynamics: hipMemset failed");
  if (rc != 0) {
    release(ctx);
    return rc;
  }
  TMD_HIP(hipDeviceSynchronize());
  return 0;
}

int tmdhip_metad_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev, const void *mass_dev,
                       double kick, double *out_dev, void *stream) {
  return side_apply(ctx, kSideMetad, "tmdhip_metad_apply", pos_dev, box_host, forces_dev, vel_dev, mass_dev, kick, out_dev, stream);
}

int tmdhip_metad_deposit(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, double height, double kdt, int plain,
                         double *log_row_dev, void *stream) {
  if (!ctx) return fail("tmdhip_metad_deposit: null context");
  MetadState *S = state_of(ctx);
  if (!S) return fail("tmdhip_metad_deposit: the context has no metadynamics (tmdhip_set_metadynamics)");
  if (!pos_dev || !box_host || !log_row_dev) return fail("tmdhip_metad_deposit: null positions, boxes or log row");
  if (!(height > 0.0) || !std::isfinite(height)) return fail("tmdhip_metad_deposit: the height must be finite and positive");
  if (!plain && (!(kdt > 0.0) || !std::isfinite(kdt))) return fail("tmdhip_metad_deposit: k_B dT must be finite and positive (or plain = 1)");
  hipStream_t st = (hipStream_t)stream;
  if (S->group_heights) {
    TMD_TRY(S->group_heights(ctx, pos_dev, box_host, height, kdt, plain, log_row_dev, st));
    return launch_deposit<double>(S, pos_dev, box_host, height, kdt, plain, log_row_dev, st, false);
  }
  return ctx->d.dtype == TMDHIP_F32 ? launch_deposit<float>(S, pos_dev, box_host, height, kdt, plain, log_row_dev, st)
                                    : launch_deposit<double>(S, pos_dev, box_host, height, kdt, plain, log_row_dev, st);
}

int tmdhip_metad_energy(tmdhip_ctx *ctx, double *out_host, void *stream) {
  return side_energy(ctx, kSideMetad, "tmdhip_metad_energy", out_host, stream);
}

int tmdhip_metad_get_grid(tmdhip_ctx *ctx, double *out_host, int64_t count) {
  if (!ctx || !out_host) return fail("tmdhip_metad_get_grid: null argument");
  MetadState *S = state_of(ctx);
  if (!S) return fail("tmdhip_metad_get_grid: the context has no metadynamics");
  if (count != (int64_t)S->grid_doubles()) return fail("tmdhip_metad_get_grid: the grid holds " + std::to_string(S->grid_doubles()) + " doubles");
  TMD_HIP(hipDeviceSynchronize());
  TMD_HIP(hipMemcpy(out_host, S->grid.p, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
  return 0;
}

int tmdhip_metad_set_grid(tmdhip_ctx *ctx, const double *in_host, int64_t count) {
  if (!ctx || !in_host) return fail("tmdhip_metad_set_grid: null argument");
  MetadState *S = state_of(ctx);
  if (!S) return fail("tmdhip_metad_set_grid: the context has no metadynamics");
  if (count != (int64_t)S->grid_doubles()) return fail("tmdhip_metad_set_grid: the grid holds " + std::to_string(S->grid_doubles()) + " doubles");
  TMD_HIP(hipDeviceSynchronize());
  TMD_HIP(hipMemcpy(S->grid.p, in_host, sizeof(double) * (size_t)count, hipMemcpyHostToDevice));
  return 0;
}

}  // extern "C"
