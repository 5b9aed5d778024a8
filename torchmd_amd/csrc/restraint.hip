// Harmonic position and distance restraints with one target per replica, for gfx950 (tmdhip_set_restraints,
// tmdhip_restraint_apply, tmdhip_restraint_energy, tmdhip_restraint_states; the per-entry arithmetic: restraint_math.h).
//
// One kernel, blockIdx.y = replica, 256 threads, ONE THREAD PER RESTRAINED ATOM: the thread walks its atom's row of a CSR built
// on the host at set-up (the position entry first, then the distance entries by restraint index), sums the row's forces in
// double in that order and is the only writer of its atom — an atom in many restraints needs no atomic, and two runs give the
// same bits.  Every distance restraint is therefore evaluated from both ends (the same d = x_i - x_j in the pair's order, so
// the two ends' forces are each other's negatives bit for bit); its energy is counted by the end with the lower atom index.
// Whatever pointer is not null is served:
//   impulse   vel only           v = R((double)v + kick F_r / m)            between two launches of tmdhip_md_run
//   finish    vel, forces, E     ... and f = R((double)f + F_r), energies   after the last step of a call
//   evaluate  forces and / or E                                             tmdhip_restraint_apply
// Arithmetic in double from positions of either dtype, one rounding on each store.  Rows of atoms in no restraint are never
// read or written.  Energies: fixed-order sum (reduce.h), the wave sums meet pairwise; a second launch of one wave per replica
// folds the blocks' two partials.  The boxes, and where each replica's positions live (inside tmdhip_md_run: either of two
// buffers), travel as kernel arguments, kSideChunk replicas per launch.
// Latency-bound: a handful of atoms, three loads deep (row -> entry -> partner position).
//
// Cross energies (tmdhip_restraint_states, for an exchange of windows between replicas): the same walk with the table
// row taken from blockIdx.z instead of the replica's own number, energies only: entry [i][k] is configuration i in box i under
// row k.  The energy lines of the two kernels are the same expressions in the same order, and both sums go through block_sums
// and fold_rows, so [i][i] has the bits restraint_kernel gives.  The partials and the result live in a workspace of their own
// (allocated at the first call): the partials and the energy row of a run are never touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.h"
#include "restraint_math.h"

using namespace tmd;

namespace {

constexpr int kThreads = 256;

struct RestraintTables {
  int natoms, nrows, npos, ndist;
  const int32_t *atom, *off;
  const RestraintEntry *ent;
  const double *pos_ref, *pos_k, *dist_r0, *dist_k;  // [R][npos][3], [R][npos], [R][ndist], [R][ndist]
};

struct RestraintState {
  int nrep = 0, natoms = 0, nrows = 0, npos = 0, ndist = 0, nblocks = 0;
  DevBuf atom, off, ent, pos_ref, pos_k, dist_r0, dist_k;
  DevBuf partials;  // double [R][nblocks][2]
  DevBuf energy;    // double [R][2]: (position, distance) of the last tmdhip_md_run
  DevBuf cross_partials, cross;  // tmdhip_restraint_states: double [R][R][nblocks][2] and [R][R][2], allocated at the first call
  std::vector<int32_t> atom_h;
  const void *mass_checked = nullptr;  // the mass array whose restrained rows are known to be positive
  void release() {
    for (DevBuf *b : {&atom, &off, &ent, &pos_ref, &pos_k, &dist_r0, &dist_k, &partials, &energy, &cross_partials, &cross}) b->release();
  }
  RestraintTables tables() const {
    return {natoms, nrows, npos, ndist, atom.as<int32_t>(), off.as<int32_t>(), ent.as<RestraintEntry>(),
            pos_ref.as<double>(), pos_k.as<double>(), dist_r0.as<double>(), dist_k.as<double>()};
  }
};

// forces / vel: the rows of the launch's first replica (blockIdx.y counts from it); rep0: that replica's index in the tables
template <typename R>
__global__ __launch_bounds__(kThreads) void restraint_kernel(RestraintTables T, R *__restrict__ forces, R *__restrict__ vel,
                                                             const R *__restrict__ mass, double kick, double *__restrict__ partials,
                                                             int nblocks, SideChunk B, int rep0) {
#pragma clang fp contract(off)
  const int r = rep0 + blockIdx.y;
  const size_t base = (size_t)blockIdx.y * T.natoms * 3;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  double energy[2] = {0.0, 0.0};  // position, distance
  if (t < T.nrows) {
    const double box[3] = {B.box[blockIdx.y][0], B.box[blockIdx.y][1], B.box[blockIdx.y][2]};
    const int a = T.atom[t];
    const R *p = (const R *)B.pos[blockIdx.y];
    const double x[3] = {(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
    double f[3] = {0.0, 0.0, 0.0};
    for (int e = T.off[t]; e < T.off[t + 1]; ++e) {
      const RestraintEntry en = T.ent[e];
      double g[3];
      if (en.kind == 0) {
        const size_t q = (size_t)r * T.npos + en.index;
        const double k = T.pos_k[q];
        if (!(k > 0.0)) continue;
        energy[0] += restraint_position(x, T.pos_ref + 3 * q, box, k, g);
        for (int c = 0; c < 3; ++c) f[c] += g[c];
      } else {
        const size_t q = (size_t)r * T.ndist + en.index;
        const double k = T.dist_k[q];
        if (!(k > 0.0)) continue;
        const int b = en.partner;
        const double y[3] = {(double)p[3 * b], (double)p[3 * b + 1], (double)p[3 * b + 2]};
        const double ed = en.sign > 0 ? restraint_distance(x, y, box, k, T.dist_r0[q], g) : restraint_distance(y, x, box, k, T.dist_r0[q], g);
        if (a < b) energy[1] += ed;
        for (int c = 0; c < 3; ++c) f[c] += en.sign > 0 ? g[c] : -g[c];
      }
    }
    side_store(forces, vel, base + 3 * (size_t)a, mass, a, kick, f);
  }
  if (!partials) return;  // (uniform: a kernel argument)
  block_sums<kThreads / 64, Meet::Pairwise>(energy, partials + ((size_t)r * nblocks + blockIdx.x) * 2);
}

// one wave per replica (blockIdx.x counts from rep0): out[r][2] = the fold of the replica's partials
__global__ __launch_bounds__(64) void restraint_fold_kernel(const double *__restrict__ partials, int nblocks, double *__restrict__ out,
                                                            int rep0) {
  const int r = rep0 + blockIdx.x;
  double sum[2];
  fold_rows(partials + (size_t)r * nblocks * 2, nblocks, sum);
  if (threadIdx.x == 0) {
    out[2 * (size_t)r] = sum[0];
    out[2 * (size_t)r + 1] = sum[1];
  }
}

// restraint_kernel's walk without the forces: blockIdx.y = configuration of the launch (rep0 counts it in), blockIdx.z = row k of
// the tables; partials [R][R][nblocks][2], (configuration, row) outermost
template <typename R>
__global__ __launch_bounds__(kThreads) void restraint_states_kernel(RestraintTables T, double *__restrict__ partials, int nblocks,
                                                                    int nrep, SideChunk B, int rep0) {
#pragma clang fp contract(off)
  const int i = rep0 + blockIdx.y, r = blockIdx.z;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  double energy[2] = {0.0, 0.0};  // position, distance
  if (t < T.nrows) {
    const double box[3] = {B.box[blockIdx.y][0], B.box[blockIdx.y][1], B.box[blockIdx.y][2]};
    const int a = T.atom[t];
    const R *p = (const R *)B.pos[blockIdx.y];
    const double x[3] = {(double)p[3 * a], (double)p[3 * a + 1], (double)p[3 * a + 2]};
    for (int e = T.off[t]; e < T.off[t + 1]; ++e) {
      const RestraintEntry en = T.ent[e];
      double g[3];
      if (en.kind == 0) {
        const size_t q = (size_t)r * T.npos + en.index;
        const double k = T.pos_k[q];
        if (!(k > 0.0)) continue;
        energy[0] += restraint_position(x, T.pos_ref + 3 * q, box, k, g);
      } else {
        const int b = en.partner;
        if (!(a < b)) continue;  // (counted by the lower atom)
        const size_t q = (size_t)r * T.ndist + en.index;
        const double k = T.dist_k[q];
        if (!(k > 0.0)) continue;
        const double y[3] = {(double)p[3 * b], (double)p[3 * b + 1], (double)p[3 * b + 2]};
        energy[1] += en.sign > 0 ? restraint_distance(x, y, box, k, T.dist_r0[q], g) : restraint_distance(y, x, box, k, T.dist_r0[q], g);
      }
    }
  }
  block_sums<kThreads / 64, Meet::Pairwise>(energy, partials + (((size_t)i * nrep + r) * nblocks + blockIdx.x) * 2);
}

// one wave per (configuration, row): out[i][k][2] = the fold of its partials
__global__ __launch_bounds__(64) void restraint_states_fold_kernel(const double *__restrict__ partials, int nblocks, double *__restrict__ out) {
  const size_t ik = blockIdx.x;
  double sum[2];
  fold_rows(partials + ik * nblocks * 2, nblocks, sum);
  if (threadIdx.x == 0) {
    out[2 * ik] = sum[0];
    out[2 * ik + 1] = sum[1];
  }
}

template <typename R>
int launch_states(RestraintState *S, const void *pos, const double *box_host, hipStream_t st) {
  const RestraintTables T = S->tables();
  const size_t stride = (size_t)S->natoms * 3;
  for (int c0 = 0; c0 < S->nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, S->nrep - c0);
    const SideChunk B = side_chunk(nr, c0, pos, nullptr, box_host, stride * sizeof(R));
    hipLaunchKernelGGL(restraint_states_kernel<R>, dim3((unsigned)S->nblocks, (unsigned)nr, (unsigned)S->nrep), dim3(kThreads), 0, st, T,
                       S->cross_partials.as<double>(), S->nblocks, S->nrep, B, c0);
  }
  hipLaunchKernelGGL(restraint_states_fold_kernel, dim3((unsigned)(S->nrep * S->nrep)), dim3(64), 0, st, S->cross_partials.as<double>(),
                     S->nblocks, S->cross.as<double>());
  TMD_HIP(hipGetLastError());
  return 0;
}

// replicas rep0 .. rep0 + nrep - 1; forces / vel point at the rows of replica rep0, box_host at its box; the positions are
// [nrep][N][3] at `pos`, or, with `pos_each`, one array per replica; `out` (double [R][2], indexed by the replica's number)
// wants the energies
template <typename R>
int launch(RestraintState *S, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces,
           void *vel, const void *mass, double kick, double *out, hipStream_t st) {
  const RestraintTables T = S->tables();
  const size_t stride = (size_t)S->natoms * 3;
  for (int c0 = 0; c0 < nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, nrep - c0);
    const SideChunk B = side_chunk(nr, c0, pos, pos_each, box_host, stride * sizeof(R));
    hipLaunchKernelGGL(restraint_kernel<R>, dim3((unsigned)S->nblocks, (unsigned)nr), dim3(kThreads), 0, st, T,
                       forces ? (R *)forces + c0 * stride : nullptr, vel ? (R *)vel + c0 * stride : nullptr,
                       (const R *)mass, kick, out ? S->partials.as<double>() : nullptr, S->nblocks, B, rep0 + c0);
  }
  if (out) hipLaunchKernelGGL(restraint_fold_kernel, dim3((unsigned)nrep), dim3(64), 0, st, S->partials.as<double>(), S->nblocks, out, rep0);
  TMD_HIP(hipGetLastError());
  return 0;
}

static_assert(kSideWidth[kSideRestraints] == 2, "restraint_fold_kernel writes (position, distance) per replica");
RestraintState *state_of(tmdhip_ctx *ctx) { return (RestraintState *)ctx->side[kSideRestraints].state; }

int launch_any(tmdhip_ctx *ctx, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces,
               void *vel, const void *mass, double kick, double *out, hipStream_t st) {
  RestraintState *S = state_of(ctx);
  return ctx->d.dtype == TMDHIP_F32 ? launch<float>(S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st)
                                    : launch<double>(S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st);
}

// a restrained atom without mass has no acceleration: refused where masses are first seen (one read-back per mass array)
int check_masses(tmdhip_ctx *ctx, const char *, const double *, const void *mass_dev, hipStream_t st) {
  RestraintState *S = state_of(ctx);
  if (!mass_dev || S->mass_checked == mass_dev) return 0;
  std::vector<char> host((size_t)ctx->real_size * S->natoms);
  TMD_HIP(hipMemcpyAsync(host.data(), mass_dev, host.size(), hipMemcpyDeviceToHost, st));
  TMD_HIP(hipStreamSynchronize(st));
  for (int32_t a : S->atom_h) {
    const double m = ctx->d.dtype == TMDHIP_F32 ? (double)((const float *)host.data())[a] : ((const double *)host.data())[a];
    if (!(m > 0.0)) return fail("restraints: atom " + std::to_string(a) + " is restrained and has no mass");
  }
  S->mass_checked = mass_dev;
  return 0;
}

double *run_energy(tmdhip_ctx *ctx) { return state_of(ctx)->energy.as<double>(); }

void release(tmdhip_ctx *ctx) {
  RestraintState *S = state_of(ctx);
  if (!S) return;
  S->release();
  delete S;
  ctx->side[kSideRestraints] = SideTerm{};
}

template <typename T>
int upload(DevBuf &b, const T *src, size_t count) {
  TMD_TRY(b.ensure(std::max<size_t>(sizeof(T) * count, 16)));
  if (count) TMD_HIP(hipMemcpy(b.p, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

extern "C" {

int tmdhip_set_restraints(tmdhip_ctx *ctx, const tmdhip_restraint_desc *desc) {
  if (!ctx || !desc) return fail("tmdhip_set_restraints: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_restraint_desc)) return fail("tmdhip_set_restraints: tmdhip_restraint_desc size mismatch (ABI)");
  if (!desc->enable || (desc->npos == 0 && desc->ndist == 0)) {
    TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the tables may still be in flight)
    release(ctx);
    return 0;
  }
  const int n = ctx->d.natoms, nrep = (int)ctx->rep.size();
  if (desc->nreplicas != nrep) return fail("tmdhip_set_restraints: nreplicas must be the context's");
  if (ctx->nactive < n) return fail("tmdhip_set_restraints: not for a context with passive atoms (a brick of the domain decomposition)");
  const std::string why = restraint_validate(n, nrep, desc->npos, desc->ndist, desc->pos_atom_host, desc->pos_ref_host, desc->pos_k_host,
                                             desc->dist_pair_host, desc->dist_r0_host, desc->dist_k_host);
  if (!why.empty()) return fail("tmdhip_set_restraints: " + why);
  std::vector<int32_t> atoms, off;
  std::vector<RestraintEntry> ent;
  restraint_build_csr(desc->npos, desc->ndist, desc->pos_atom_host, desc->dist_pair_host, atoms, off, ent);
  if (ctx->vsites) {
    const VsiteState *V = (const VsiteState *)ctx->vsites;
    for (int32_t s : V->site_h)
      if (std::binary_search(atoms.begin(), atoms.end(), s))
        return fail("tmdhip_set_restraints: atom " + std::to_string(s) + " is a virtual site (restrain its parents)");
  }
  TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the old tables may still be in flight)
  RestraintState *S = state_of(ctx);
  if (!S) ctx->side[kSideRestraints] = SideTerm{S = new RestraintState, "restraints need", launch_any, check_masses, run_energy, release};
  const bool same_atoms = S->atom_h == atoms;
  S->nrep = nrep;
  S->natoms = n;
  S->nrows = (int)atoms.size();
  S->npos = desc->npos;
  S->ndist = desc->ndist;
  S->nblocks = (S->nrows + kThreads - 1) / kThreads;
  S->atom_h = atoms;
  if (!same_atoms) S->mass_checked = nullptr;
  const size_t np = (size_t)nrep * desc->npos, nd = (size_t)nrep * desc->ndist;
  int rc = upload(S->atom, atoms.data(), atoms.size());
  if (rc == 0) rc = upload(S->off, off.data(), off.size());
  if (rc == 0) rc = upload(S->ent, ent.data(), ent.size());
  if (rc == 0) rc = upload(S->pos_ref, desc->pos_ref_host, 3 * np);
  if (rc == 0) rc = upload(S->pos_k, desc->pos_k_host, np);
  if (rc == 0) rc = upload(S->dist_r0, desc->dist_r0_host, nd);
  if (rc == 0) rc = upload(S->dist_k, desc->dist_k_host, nd);
  if (rc == 0) rc = S->partials.ensure(sizeof(double) * 2 * (size_t)nrep * S->nblocks);
  if (rc == 0 && S->energy.bytes < sizeof(double) * kSideWidth[kSideRestraints] * (size_t)nrep) {
    rc = S->energy.ensure(sizeof(double) * kSideWidth[kSideRestraints] * (size_t)nrep);
    if (rc == 0 && hipMemset(S->energy.p, 0, S->energy.bytes) != hipSuccess) rc = fail("tmdhip_set_restraints: hipMemset failed");
  }
  if (rc != 0) {
    release(ctx);
    return rc;
  }
  TMD_HIP(hipDeviceSynchronize());
  return 0;
}

int tmdhip_restraint_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev,
                           const void *mass_dev, double kick, double *energies_dev, void *stream) {
  return side_apply(ctx, kSideRestraints, "tmdhip_restraint_apply", pos_dev, box_host, forces_dev, vel_dev, mass_dev, kick, energies_dev,
                    stream);
}

int tmdhip_restraint_energy(tmdhip_ctx *ctx, double *out_host, void *stream) {
  return side_energy(ctx, kSideRestraints, "tmdhip_restraint_energy", out_host, stream);
}

int tmdhip_restraint_states(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, double *out_host, void *stream) {
  if (!ctx || !pos_dev || !box_host || !out_host) return fail("tmdhip_restraint_states: null argument");
  RestraintState *S = state_of(ctx);
  const size_t nrep = ctx->rep.size(), count = 2 * nrep * nrep;
  if (!S) {
    std::fill(out_host, out_host + count, 0.0);
    return 0;
  }
  if (nrep > 65535) return fail("tmdhip_restraint_states: at most 65535 replicas (the table row is a grid axis)");
  hipStream_t st = (hipStream_t)stream;
  // (a buffer that grows is freed: nothing of an earlier call is in flight, every call ends with a synchronisation)
  TMD_TRY(S->cross_partials.ensure(sizeof(double) * count * S->nblocks));
  TMD_TRY(S->cross.ensure(sizeof(double) * count));
  TMD_TRY(ctx->d.dtype == TMDHIP_F32 ? launch_states<float>(S, pos_dev, box_host, st) : launch_states<double>(S, pos_dev, box_host, st));
  TMD_HIP(hipMemcpyAsync(out_host, S->cross.p, sizeof(double) * count, hipMemcpyDeviceToHost, st));
  TMD_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
