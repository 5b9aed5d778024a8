// Metadynamics on CVs of groups of atoms, for gfx950 (tmdhip_set_metadynamics_groups; the arithmetic: cv_math.h; the grid side,
// the node kernel and every other entry point: metad.hip, which serves both flavours from slot kSideMetad).
//
// An application is TWO DEPENDENT LAUNCHES, blocks of 256 threads, arithmetic in double from positions of either dtype:
//   gather   grid (G + tasks, replicas of the launch).  Block g < G is group_restraint.hip's centre block: thread t takes
//            members t, t + 256, ... of group g, the three weighted sums go through the fixed-order sum of reduce.h, thread
//            c < 3 stores x_a0[c] + sum[c] into the context-owned centres, double [R][G][3].  Every further block is one task
//            of a coordination CV, all pairs, tiled, no cutoff list: its lanes stand for 256 atoms of one set, a split of the
//            other set streams through LDS 256 atoms at a time and is read as broadcasts (every lane the same address).  A
//            lane sums its own f and its own gradient and is the only writer of its row (split, lane) of the gradient scratch.
//            Each CV has two passes, lanes = A and lanes = B, so both sets get their gradients without a second launch; the
//            pass with more lanes also sends its values through block_sums into the replica's partial rows.  A set of few
//            atoms against many (an ion and its solvent) is cut into splits so that its few lanes do not walk the whole
//            stream alone; the scatter adds a lane's splits in ascending order.
//   scatter  grid (blocks of distinct CV atoms, replicas).  Wave 0 of every block folds the partial rows (fold_rows), thread 0
//            forms s from the fold or from the centres, V and dV/ds with metad_interp on the replica's grid, and leaves dV and
//            ds/dX in LDS: every block computes the same bits.  Then one thread per distinct atom walks its entries (CV order;
//            within a centre CV by ascending group, within a coordination CV lanes = A before lanes = B), F_a = -sum_c dV_c
//            ds_c/dx_a, and is the only writer of its atom (side_store): impulse, finish or evaluate, whatever pointer is not
//            null.  Thread 0 of block 0 writes (V, s_0, s_1) where a report is wanted.
// Two, because s needs every pair and every member before the first force can be formed, and one kernel cannot wait for all
// its blocks.  A deposition is gather -> heights (one wave per replica: the same fold and CVs, V on the grid as it is, the log
// row) -> metad.hip's node kernel.  No floating-point atomics, no host synchronisation; rows of atoms in no CV are never read
// or written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "cv_math.h"
#include "engine.h"
#include "metad_state.h"
#include "reduce.h"

using namespace tmd;

namespace {

constexpr int kThreads = kCvThreads;
constexpr int kSplitBatch = 16;  // rows of an atom's splits the scatter loads before it adds them

struct CvDevTables {
  int natoms, ngroups, ncv, nrows, npart_rows;
  int64_t grad_doubles;
  int32_t kind[kMetadMaxCv], groups[kMetadMaxCv][4], part_off[kMetadMaxCv], part_n[kMetadMaxCv];
  CoordParams coord[kMetadMaxCv];
  const int32_t *group_off, *member_atom;
  const double *member_w;
  const CvPass *pass;
  const CvTask *task;
  const int32_t *atom, *ent_off;
  const CvEntry *ent;
  double *centres;   // [R][G][3]
  double *grad;      // [R][grad_doubles]
  double *partials;  // [R][npart_rows]
};

struct CvGroupState {
  CvDevTables T{};
  int ntasks = 0, nblocks_rows = 0;
  std::vector<int32_t> atom_h;
  DevBuf group_off, member_atom, member_w, pass, task, atom, ent_off, ent, centres, grad, partials;
  void release() {
    for (DevBuf *b : {&group_off, &member_atom, &member_w, &pass, &task, &atom, &ent_off, &ent, &centres, &grad, &partials}) b->release();
  }
};

// grid (G + tasks, replicas of the launch); rep0: the first replica's index in the context-owned buffers
template <typename R>
__global__ __launch_bounds__(kThreads) void cv_gather_kernel(CvDevTables T, SideChunk B, int rep0) {
#pragma clang fp contract(off)
  __shared__ double tile[kThreads][3];
  __shared__ int tile_atom[kThreads];
  const int r = rep0 + blockIdx.y;
  const double box[3] = {B.box[blockIdx.y][0], B.box[blockIdx.y][1], B.box[blockIdx.y][2]};
  const R *p = (const R *)B.pos[blockIdx.y];
  if ((int)blockIdx.x < T.ngroups) {
    const int g = blockIdx.x;
    const int m0 = T.group_off[g], m1 = T.group_off[g + 1];
    const int a0 = T.member_atom[m0];
    const double x0[3] = {(double)p[3 * (size_t)a0], (double)p[3 * (size_t)a0 + 1], (double)p[3 * (size_t)a0 + 2]};
    double acc[3] = {0.0, 0.0, 0.0};
    for (int m = m0 + (int)threadIdx.x; m < m1; m += kThreads) {
      const size_t a = (size_t)T.member_atom[m];
      const double x[3] = {(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
      group_centre_add(x, x0, box, T.member_w[m], acc);
    }
    double s[3];
    for (int c = 0; c < 3; ++c) s[c] = wave_sum(acc[c]);
    const double sum = meet_in_lds<Meet::Pairwise, 3, Sum>(s);
    const double first = threadIdx.x == 0 ? x0[0] : (threadIdx.x == 1 ? x0[1] : x0[2]);
    if (threadIdx.x < 3) T.centres[((size_t)r * T.ngroups + g) * 3 + threadIdx.x] = first + sum;
    return;
  }
  const CvTask task = T.task[blockIdx.x - T.ngroups];
  const CvPass P = T.pass[task.pass];
  const CoordParams C = T.coord[P.cv];
  const int i = task.block * kThreads + (int)threadIdx.x;
  const bool live = i < P.nlane;
  int ai = -1;
  double xi[3] = {0.0, 0.0, 0.0};
  if (live) {
    ai = T.member_atom[P.lane0 + i];
    for (int c = 0; c < 3; ++c) xi[c] = (double)p[3 * (size_t)ai + c];
  }
  double val = 0.0, grad[3] = {0.0, 0.0, 0.0};
  const int j0 = task.split * P.chunk, j1 = min(P.nstream, j0 + P.chunk);
  for (int base = j0; base < j1; base += kThreads) {
    const int j = base + (int)threadIdx.x;
    if (j < j1) {
      const int aj = T.member_atom[P.stream0 + j];
      tile_atom[threadIdx.x] = aj;
      for (int c = 0; c < 3; ++c) tile[threadIdx.x][c] = (double)p[3 * (size_t)aj + c];
    }
    __syncthreads();
    const int n = min(kThreads, j1 - base);
    if (live)
      for (int k = 0; k < n; ++k) {
        if (tile_atom[k] == ai) continue;  // (an atom of both sets, against itself)
        const double xj[3] = {tile[k][0], tile[k][1], tile[k][2]};
        coord_pair_add(C, xi, xj, box, val, grad);
      }
    __syncthreads();
  }
  if (live) {
    double *g = T.grad + (size_t)r * T.grad_doubles + P.grad_off + ((size_t)task.split * P.nlane + i) * 3;
    for (int c = 0; c < 3; ++c) g[c] = grad[c];
  }
  if (P.value) {  // (uniform in the block)
    const double v[1] = {val};
    block_sums<kThreads / 64, Meet::Pairwise>(v, T.partials + (size_t)r * T.npart_rows + P.part_off + task.block * P.nsplit + task.split);
  }
}

// The CVs of replica r from the gather's output, by one wave (every lane returns the same): s[c] and, for a CV of centres,
// g[c][place][3] = ds/dX
__device__ __forceinline__ void cv_values(const CvDevTables &T, int r, const double *box, double (&s)[kMetadMaxCv],
                                          double (&g)[kMetadMaxCv][4][3]) {
  for (int c = 0; c < kMetadMaxCv; ++c) {
    s[c] = 0.0;
    for (int a = 0; a < 4; ++a) g[c][a][0] = g[c][a][1] = g[c][a][2] = 0.0;
    if (c >= T.ncv) continue;
    if (T.kind[c] == kCvCoordination) {
      double sum[1];
      fold_rows(T.partials + (size_t)r * T.npart_rows + T.part_off[c], T.part_n[c], sum);
      s[c] = sum[0];
      continue;
    }
    double X[4][3];
    for (int a = 0; a < 4; ++a) {
      const int gi = a < cv_arity(T.kind[c]) ? T.groups[c][a] : -1;
      for (int k = 0; k < 3; ++k) X[a][k] = gi >= 0 ? T.centres[((size_t)r * T.ngroups + gi) * 3 + k] : 0.0;
    }
    s[c] = cv_of_centres(T.kind[c], X, box, g[c]);
  }
}

// grid (blocks of rows, replicas of the launch); forces / vel: the rows of the launch's first replica
template <typename R>
__global__ __launch_bounds__(kThreads) void cv_scatter_kernel(CvDevTables T, MetadDef D, const double *__restrict__ grid, size_t grid_stride,
                                                              R *__restrict__ forces, R *__restrict__ vel, const R *__restrict__ mass,
                                                              double kick, double *__restrict__ out, SideChunk B, int rep0) {
#pragma clang fp contract(off)
  __shared__ double sh_dV[kMetadMaxCv];
  __shared__ double sh_g[kMetadMaxCv][4][3];
  const int r = rep0 + blockIdx.y;
  if (threadIdx.x < 64) {
    const double box[3] = {B.box[blockIdx.y][0], B.box[blockIdx.y][1], B.box[blockIdx.y][2]};
    double s[kMetadMaxCv], g[kMetadMaxCv][4][3], dV[kMetadMaxCv];
    cv_values(T, r, box, s, g);
    if (threadIdx.x == 0) {
      const double V = metad_interp(D, grid + (size_t)r * grid_stride, s, dV);
      for (int c = 0; c < kMetadMaxCv; ++c) {
        sh_dV[c] = dV[c];
        for (int a = 0; a < 4; ++a)
          for (int k = 0; k < 3; ++k) sh_g[c][a][k] = g[c][a][k];
      }
      if (out && blockIdx.x == 0) {
        out[(size_t)r * kMetadOut] = V;
        for (int c = 0; c < kMetadMaxCv; ++c) out[(size_t)r * kMetadOut + 1 + c] = s[c];
      }
    }
  }
  __syncthreads();
  const int t = blockIdx.x * kThreads + (int)threadIdx.x;
  if (t >= T.nrows || (!forces && !vel)) return;
  const int a = T.atom[t];
  const double *G = T.grad + (size_t)r * T.grad_doubles;
  double f[3] = {0.0, 0.0, 0.0};
  int e = T.ent_off[t];
  const int e1 = T.ent_off[t + 1];
  for (int c = 0; c < T.ncv; ++c) {
    double ds[3] = {0.0, 0.0, 0.0};  // ds_c / dx_a
    bool any = false;
    for (; e < e1; ++e) {
      const CvEntry E = T.ent[e];
      if (E.cv != c) break;
      any = true;
      if (E.type == 0) {
        for (int k = 0; k < 3; ++k) ds[k] += E.w * sh_g[c][E.at][k];
      } else {
        // the splits in ascending order; sixteen rows are loaded before they are added, so that a small set's hundreds of
        // splits cost one load latency per sixteen and not one each (the additions and their order are the same)
        double part[3] = {0.0, 0.0, 0.0};
        for (int q0 = 0; q0 < E.nsplit; q0 += kSplitBatch) {
          double row[kSplitBatch][3];
#pragma unroll
          for (int u = 0; u < kSplitBatch; ++u)
            for (int k = 0; k < 3; ++k) row[u][k] = q0 + u < E.nsplit ? G[(size_t)E.at + (size_t)(q0 + u) * E.stride + k] : 0.0;
#pragma unroll
          for (int u = 0; u < kSplitBatch; ++u)
            if (q0 + u < E.nsplit)
              for (int k = 0; k < 3; ++k) part[k] += row[u][k];
        }
        for (int k = 0; k < 3; ++k) ds[k] += part[k];
      }
    }
    if (any)
      for (int k = 0; k < 3; ++k) f[k] += -sh_dV[c] * ds[k];
  }
  side_store(forces, vel, ((size_t)blockIdx.y * T.natoms + (size_t)a) * 3, mass, a, kick, f);
}

// (a) of the deposit chain behind a gather: one wave per replica, row[r] = (s0..., w) with V(s0) read from the grid as it is
__global__ __launch_bounds__(64) void cv_height_kernel(CvDevTables T, MetadDef D, const double *__restrict__ grid, size_t grid_stride,
                                                       double height, double kdt, int plain, double *__restrict__ row, SideChunk B, int rep0) {
#pragma clang fp contract(off)
  const int r = rep0 + blockIdx.x;
  const double box[3] = {B.box[blockIdx.x][0], B.box[blockIdx.x][1], B.box[blockIdx.x][2]};
  double s[kMetadMaxCv], g[kMetadMaxCv][4][3], dV[kMetadMaxCv];
  cv_values(T, r, box, s, g);
  if (threadIdx.x != 0) return;
  const double V = metad_interp(D, grid + (size_t)r * grid_stride, s, dV);
  double *o = row + (size_t)r * (D.ncv + 1);
  for (int c = 0; c < D.ncv; ++c) o[c] = s[c];
  o[D.ncv] = metad_height(height, V, kdt, plain);
}

MetadState *state_of(tmdhip_ctx *ctx) { return metad_state_of(ctx); }
CvGroupState *group_of(MetadState *S) { return (CvGroupState *)S->group; }

template <typename R>
void launch_gather(MetadState *S, int nr, const SideChunk &B, int rep, hipStream_t st) {
  CvGroupState *Q = group_of(S);
  hipLaunchKernelGGL(cv_gather_kernel<R>, dim3((unsigned)(Q->T.ngroups + Q->ntasks), (unsigned)nr), dim3(kThreads), 0, st, Q->T, B, rep);
}

// arguments as SideTerm::launch
template <typename R>
int launch(MetadState *S, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces, void *vel,
           const void *mass, double kick, double *out, hipStream_t st) {
  CvGroupState *Q = group_of(S);
  const size_t stride = (size_t)S->natoms * 3;
  const size_t gstride = S->shared ? 0 : (size_t)S->nodes * metad_width(S->def);
  for (int c0 = 0; c0 < nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, nrep - c0);
    const SideChunk B = side_chunk(nr, c0, pos, pos_each, box_host, stride * sizeof(R));
    launch_gather<R>(S, nr, B, rep0 + c0, st);
    hipLaunchKernelGGL(cv_scatter_kernel<R>, dim3((unsigned)Q->nblocks_rows, (unsigned)nr), dim3(kThreads), 0, st, Q->T, S->def,
                       S->grid.as<double>(), gstride, forces ? (R *)forces + c0 * stride : nullptr, vel ? (R *)vel + c0 * stride : nullptr,
                       (const R *)mass, kick, out, B, rep0 + c0);
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

int launch_any(tmdhip_ctx *ctx, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces,
               void *vel, const void *mass, double kick, double *out, hipStream_t st) {
  MetadState *S = state_of(ctx);
  return ctx->d.dtype == TMDHIP_F32 ? launch<float>(S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st)
                                    : launch<double>(S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st);
}

template <typename R>
int launch_heights(MetadState *S, const void *pos, const double *box_host, double height, double kdt, int plain, double *row,
                   hipStream_t st) {
  CvGroupState *Q = group_of(S);
  const size_t stride = (size_t)S->natoms * 3;
  const size_t gstride = S->shared ? 0 : (size_t)S->nodes * metad_width(S->def);
  for (int c0 = 0; c0 < S->nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, S->nrep - c0);
    const SideChunk B = side_chunk(nr, c0, pos, nullptr, box_host, stride * sizeof(R));
    launch_gather<R>(S, nr, B, c0, st);
    hipLaunchKernelGGL(cv_height_kernel, dim3((unsigned)nr), dim3(64), 0, st, Q->T, S->def, S->grid.as<double>(), gstride, height, kdt,
                       plain, row, B, c0);
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

// what a deposition refuses of its boxes, then the gather and the heights
int heights_any(tmdhip_ctx *ctx, const void *pos, const double *box_host, double height, double kdt, int plain, double *row, hipStream_t st) {
  MetadState *S = state_of(ctx);
  CvGroupState *Q = group_of(S);
  for (int c = 0; c < Q->T.ncv; ++c)
    if (Q->T.kind[c] == kCvCoordination)
      for (int r = 0; r < S->nrep; ++r) {
        const std::string why = cv_check_box(Q->T.coord[c], box_host + 3 * r);
        if (!why.empty()) return fail("tmdhip_metad_deposit: CV " + std::to_string(c) + ": " + why);
      }
  return ctx->d.dtype == TMDHIP_F32 ? launch_heights<float>(S, pos, box_host, height, kdt, plain, row, st)
                                    : launch_heights<double>(S, pos, box_host, height, kdt, plain, row, st);
}

// A coordination CV without dmax, or with dmax beyond half the shortest non-zero edge, in a periodic box; and a CV atom
// without mass, which has no acceleration: refused where masses are first seen (one read-back per mass array)
int run_check(tmdhip_ctx *ctx, const char *who, const double *box_host, const void *mass_dev, hipStream_t st) {
  MetadState *S = state_of(ctx);
  CvGroupState *Q = group_of(S);
  if (box_host)
    for (int c = 0; c < Q->T.ncv; ++c)
      if (Q->T.kind[c] == kCvCoordination)
        for (int r = 0; r < S->nrep; ++r) {
          const std::string why = cv_check_box(Q->T.coord[c], box_host + 3 * r);
          if (!why.empty()) return fail(std::string(who ? who : "metadynamics") + ": metadynamics: CV " + std::to_string(c) + ": " + why);
        }
  if (!mass_dev || S->mass_checked == mass_dev) return 0;
  std::vector<char> host((size_t)ctx->real_size * S->natoms);
  TMD_HIP(hipMemcpyAsync(host.data(), mass_dev, host.size(), hipMemcpyDeviceToHost, st));
  TMD_HIP(hipStreamSynchronize(st));
  for (int32_t a : Q->atom_h) {
    const double m = ctx->d.dtype == TMDHIP_F32 ? (double)((const float *)host.data())[a] : ((const double *)host.data())[a];
    if (!(m > 0.0)) return fail(std::string(who ? who : "metadynamics") + ": metadynamics: atom " + std::to_string(a) + " belongs to a CV and has no mass");
  }
  S->mass_checked = mass_dev;
  return 0;
}

void release_group(MetadState *S) {
  CvGroupState *Q = group_of(S);
  if (!Q) return;
  Q->release();
  delete Q;
  S->group = nullptr;
}

template <typename T>
int upload(DevBuf &b, const std::vector<T> &src) {
  TMD_TRY(b.ensure(std::max<size_t>(sizeof(T) * src.size(), 16)));
  if (!src.empty()) TMD_HIP(hipMemcpy(b.p, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

extern "C" {

int tmdhip_set_metadynamics_groups(tmdhip_ctx *ctx, const tmdhip_metad_group_desc *desc) {
  const std::string who = "tmdhip_set_metadynamics_groups: ";
  if (!ctx || !desc) return fail(who + "null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_metad_group_desc)) return fail(who + "tmdhip_metad_group_desc size mismatch (ABI)");
  if (!desc->enable) {
    TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the grid may still be in flight)
    if (ctx->side[kSideMetad].state) ctx->side[kSideMetad].release(ctx);
    return 0;
  }
  const int n = ctx->d.natoms, nrep = (int)ctx->rep.size();
  if (desc->nreplicas != nrep) return fail(who + "nreplicas must be the context's");
  if (ctx->nactive < n) return fail(who + "not for a context with passive atoms (a brick of the domain decomposition)");
  const int G = desc->ngroups;
  const std::string why = cv_validate(n, desc->ncv, desc->kind, &desc->groups[0][0], G, desc->group_off_host, desc->member_atom_host,
                                      desc->member_weight_host, desc->bins, desc->grid_min, desc->grid_max, desc->sigma, desc->coord_n,
                                      desc->coord_r0, desc->coord_d0, desc->coord_dmax);
  if (!why.empty()) return fail(who + why);
  std::vector<double> w;
  group_normalise(G, desc->group_off_host, desc->member_weight_host, w);
  const CvTables H = cv_build(desc->ncv, desc->kind, &desc->groups[0][0], G, desc->group_off_host, desc->member_atom_host, w);
  if (ctx->vsites) {
    const VsiteState *V = (const VsiteState *)ctx->vsites;
    for (int32_t a : H.atom)
      if (std::find(V->site_h.begin(), V->site_h.end(), a) != V->site_h.end())
        return fail(who + "atom " + std::to_string(a) + " is a virtual site (use its parents)");
  }
  TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the old grid may still be in flight)
  if (ctx->side[kSideMetad].state) ctx->side[kSideMetad].release(ctx);
  MetadState *S = new MetadState;
  CvGroupState *Q = new CvGroupState;
  S->group = Q;
  S->group_heights = heights_any;
  S->group_release = release_group;
  ctx->side[kSideMetad] = SideTerm{S, "metadynamics needs", launch_any, run_check, metad_run_energy, metad_release};
  S->nrep = nrep;
  S->natoms = n;
  S->shared = desc->shared ? 1 : 0;
  S->def = cv_grid_define(desc->ncv, desc->kind, desc->bins, desc->grid_min, desc->grid_max, desc->sigma);
  S->nodes = metad_nodes(S->def);
  S->ngrids = S->shared ? 1 : nrep;
  const size_t nm = (size_t)desc->group_off_host[G];
  int rc = upload(Q->group_off, std::vector<int32_t>(desc->group_off_host, desc->group_off_host + G + 1));
  if (rc == 0) rc = upload(Q->member_atom, std::vector<int32_t>(desc->member_atom_host, desc->member_atom_host + nm));
  if (rc == 0) rc = upload(Q->member_w, w);
  if (rc == 0) rc = upload(Q->pass, H.pass);
  if (rc == 0) rc = upload(Q->task, H.task);
  if (rc == 0) rc = upload(Q->atom, H.atom);
  if (rc == 0) rc = upload(Q->ent_off, H.ent_off);
  if (rc == 0) rc = upload(Q->ent, H.ent);
  if (rc == 0) rc = Q->centres.ensure(sizeof(double) * 3 * (size_t)nrep * G);
  if (rc == 0) rc = Q->grad.ensure(std::max<size_t>(sizeof(double) * (size_t)nrep * H.grad_doubles, 16));
  if (rc == 0) rc = Q->partials.ensure(std::max<size_t>(sizeof(double) * (size_t)nrep * H.part_rows, 16));
  if (rc == 0) rc = S->grid.ensure(sizeof(double) * S->grid_doubles());
  if (rc == 0) rc = S->last.ensure(sizeof(double) * kMetadOut * (size_t)nrep);
  if (rc == 0 && (hipMemset(S->grid.p, 0, S->grid.bytes) != hipSuccess || hipMemset(S->last.p, 0, S->last.bytes) != hipSuccess))
    rc = fail(who + "hipMemset failed");
  if (rc != 0) {
    metad_release(ctx);
    return rc;
  }
  Q->atom_h = H.atom;
  Q->ntasks = (int)H.task.size();
  Q->nblocks_rows = ((int)H.atom.size() + kThreads - 1) / kThreads;
  CvDevTables &T = Q->T;
  T.natoms = n;
  T.ngroups = G;
  T.ncv = desc->ncv;
  T.nrows = (int)H.atom.size();
  T.npart_rows = (int)H.part_rows;
  T.grad_doubles = H.grad_doubles;
  for (int c = 0; c < kMetadMaxCv; ++c) {
    T.kind[c] = c < desc->ncv ? desc->kind[c] : 0;
    for (int a = 0; a < 4; ++a) T.groups[c][a] = c < desc->ncv ? desc->groups[c][a] : -1;
    T.part_off[c] = H.part_off[c];
    T.part_n[c] = H.part_n[c];
    T.coord[c] = (c < desc->ncv && desc->kind[c] == kCvCoordination)
                     ? coord_params(desc->coord_r0[c], desc->coord_n[c], desc->coord_d0[c], desc->coord_dmax[c])
                     : CoordParams{};
  }
  T.group_off = Q->group_off.as<int32_t>();
  T.member_atom = Q->member_atom.as<int32_t>();
  T.member_w = Q->member_w.as<double>();
  T.pass = Q->pass.as<CvPass>();
  T.task = Q->task.as<CvTask>();
  T.atom = Q->atom.as<int32_t>();
  T.ent_off = Q->ent_off.as<int32_t>();
  T.ent = Q->ent.as<CvEntry>();
  T.centres = Q->centres.as<double>();
  T.grad = Q->grad.as<double>();
  T.partials = Q->partials.as<double>();
  TMD_HIP(hipDeviceSynchronize());
  return 0;
}

}  // extern "C"
