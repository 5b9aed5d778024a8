// Harmonic, optionally flat-bottomed restraints on the distance, angle and dihedral between centres of groups of atoms, with
// targets, strengths and widths per replica, for gfx950 (tmdhip_set_group_restraints, tmdhip_group_restraint_apply,
// tmdhip_group_restraint_energy, tmdhip_group_restraint_states; the arithmetic: group_math.h).  The fifth side term.
//
// Three kernels, blockIdx.y = replica of the launch, 256 threads, arithmetic in double from positions of either dtype:
//   centres   ONE BLOCK PER (GROUP, REPLICA): thread t takes members t, t + 256, ... of the group in that order, the three
//             weighted sums go through the fixed-order sum of reduce.h (butterfly, pairwise meet), thread c < 3 stores
//             x_a0[c] + sum[c] into the context-owned centres, double [R][G][3].
//   forces    ONE THREAD PER DISTINCT ATOM that belongs to a group some restraint names: it walks its memberships by ascending
//             group, per group the restraints that name it by ascending index, takes each restraint's force on the group's
//             centre (recomputed from the centres, a handful of loads: once per block into LDS for up to 256 restraints, by
//             the thread itself beyond that), and is the only writer of its atom: F_a = sum_g w_a G_g.
//             Whatever pointer is not null is served (side_store): vel (the impulse), vel + forces (the finish), forces.
//   energies  only where energies are wanted: one thread per restraint, block_sums with the pairwise meet, then a fold of one
//             wave per replica.  Row (distance, angle, dihedral).
// No floating-point atomics: two runs give the same bits.  Rows of atoms in no group are never read or written.  The boxes and
// where each replica's positions live travel as kernel arguments (SideChunk), kSideChunk replicas per launch.
// Latency-bound: an application inside tmdhip_md_run is two dependent launches of a few blocks.
//
// Cross energies (tmdhip_group_restraint_states): the centres of every configuration, then the energy kernel's walk with the
// table row taken from blockIdx.z: the same device function in both, both sums through block_sums and fold_rows, so [i][i]
// has the bits of the run's energy row.  Partials and result live in a workspace of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.h"
#include "group_math.h"

using namespace tmd;

namespace {

constexpr int kThreads = 256;
constexpr int kWidth = 3;

struct GroupTables {
  int natoms, ngroups, nrest, nrows;
  const int32_t *group_off, *member_atom;  // [G + 1], [members]
  const double *member_w;                  // normalised
  const int32_t *kind, *groups;            // [M], [M][4]
  const int32_t *use_off;                  // [G + 1]
  const GroupUse *use;
  const int32_t *atom, *mem_off;  // [nrows], [nrows + 1]
  const GroupMember *mem;
  const double *target, *k, *flat;  // [R][M]
  double *centres;                  // [R][G][3]
};

struct GroupState {
  int nrep = 0, natoms = 0, ngroups = 0, nrest = 0, nrows = 0, nblocks_a = 0, nblocks_m = 0;
  DevBuf group_off, member_atom, member_w, kind, groups, use_off, use, atom, mem_off, mem, target, k, flat, centres;
  DevBuf partials;               // double [R][nblocks_m][3]
  DevBuf energy;                 // double [R][3] of the last tmdhip_md_run
  DevBuf cross_partials, cross;  // double [R][R][nblocks_m][3] and [R][R][3], allocated at the first call
  std::vector<int32_t> atom_h;
  const void *mass_checked = nullptr;
  void release() {
    for (DevBuf *b : {&group_off, &member_atom, &member_w, &kind, &groups, &use_off, &use, &atom, &mem_off, &mem, &target, &k, &flat,
                      &centres, &partials, &energy, &cross_partials, &cross})
      b->release();
  }
  GroupTables tables() const {
    return {natoms, ngroups, nrest, nrows, group_off.as<int32_t>(), member_atom.as<int32_t>(), member_w.as<double>(), kind.as<int32_t>(),
            groups.as<int32_t>(), use_off.as<int32_t>(), use.as<GroupUse>(), atom.as<int32_t>(), mem_off.as<int32_t>(),
            mem.as<GroupMember>(), target.as<double>(), k.as<double>(), flat.as<double>(), centres.as<double>()};
  }
};

// grid (G, replicas of the launch); rep0: the first replica's index in the tables and in the centres
template <typename R>
__global__ __launch_bounds__(kThreads) void group_centre_kernel(GroupTables T, SideChunk B, int rep0) {
#pragma clang fp contract(off)
  const int g = blockIdx.x, r = rep0 + blockIdx.y;
  const double box[3] = {B.box[blockIdx.y][0], B.box[blockIdx.y][1], B.box[blockIdx.y][2]};
  const R *p = (const R *)B.pos[blockIdx.y];
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
}

// restraint m of table row `row` on the centres X (double [G][3]): the energy, and the forces on its centres
__device__ __forceinline__ double group_eval(const GroupTables &T, const double *__restrict__ X, const double *box, int row, int m,
                                             double (&F)[4][3], bool &on) {
  const size_t q = (size_t)row * T.nrest + m;
  const double k = T.k[q];
  on = k > 0.0;
  if (!on) return 0.0;
  const int kind = T.kind[m];
  double C[4][3];
  for (int a = 0; a < 4; ++a) {
    const int g = a < group_arity(kind) ? T.groups[4 * m + a] : -1;
    for (int c = 0; c < 3; ++c) C[a][c] = g >= 0 ? X[3 * (size_t)g + c] : 0.0;
  }
  return group_restraint(kind, C, box, T.target[q], k, T.flat[q], F);
}

// restraints a block of the force kernel evaluates once into LDS (12 doubles each: 24 KB); a set with more is recomputed per atom
constexpr int kLdsRestraints = kThreads;

// forces / vel: the rows of the launch's first replica (blockIdx.y counts from it).  With at most kLdsRestraints restraints
// every block first evaluates them all, thread m restraint m, into LDS, and the atoms' threads read the forces on their
// groups' centres from there: the same values added in the same order as by the thread that recomputes them itself, but an
// atom in five restraints no longer walks five chains of dependent loads one after the other.
template <typename R>
__global__ __launch_bounds__(kThreads) void group_force_kernel(GroupTables T, R *__restrict__ forces, R *__restrict__ vel,
                                                               const R *__restrict__ mass, double kick, SideChunk B, int rep0) {
#pragma clang fp contract(off)
  __shared__ double centre_force[kLdsRestraints][12];
  __shared__ int active[kLdsRestraints];
  const int r = rep0 + blockIdx.y;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  const double box[3] = {B.box[blockIdx.y][0], B.box[blockIdx.y][1], B.box[blockIdx.y][2]};
  const double *X = T.centres + (size_t)r * T.ngroups * 3;
  const bool in_lds = T.nrest <= kLdsRestraints;  // (uniform: a kernel argument)
  int e0 = 0, e1 = 0;
  if (t < T.nrows) {
    e0 = T.mem_off[t];
    e1 = T.mem_off[t + 1];
  }
  if (in_lds) {
    if ((int)threadIdx.x < T.nrest) {
      double F[4][3];
      bool on;
      group_eval(T, X, box, r, (int)threadIdx.x, F, on);
      active[threadIdx.x] = on ? 1 : 0;
      for (int q = 0; q < 4; ++q)
        for (int c = 0; c < 3; ++c) centre_force[threadIdx.x][3 * q + c] = on ? F[q][c] : 0.0;
    }
    __syncthreads();
  }
  if (t >= T.nrows) return;
  const int a = T.atom[t];
  double f[3] = {0.0, 0.0, 0.0};
  for (int e = e0; e < e1; ++e) {
    const GroupMember me = T.mem[e];
    double G[3] = {0.0, 0.0, 0.0};
    for (int u = T.use_off[me.group]; u < T.use_off[me.group + 1]; ++u) {
      const GroupUse us = T.use[u];
      if (in_lds) {
        if (!active[us.index]) continue;
        for (int c = 0; c < 3; ++c) G[c] += centre_force[us.index][3 * us.role + c];
        continue;
      }
      double F[4][3];
      bool on;
      group_eval(T, X, box, r, us.index, F, on);
      if (!on) continue;
      for (int q = 0; q < 4; ++q)
        if (q == us.role)
          for (int c = 0; c < 3; ++c) G[c] += F[q][c];
    }
    const double w = T.member_w[me.member];
    for (int c = 0; c < 3; ++c) f[c] += w * G[c];
  }
  side_store(forces, vel, ((size_t)blockIdx.y * T.natoms + (size_t)a) * 3, mass, a, kick, f);
}

// the lane's restraint under table row `row`, by kind
__device__ __forceinline__ void group_energy_lane(const GroupTables &T, const double *__restrict__ X, const double *box, int row,
                                                  double (&energy)[kWidth]) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  energy[0] = energy[1] = energy[2] = 0.0;
  if (m >= T.nrest) return;
  double F[4][3];
  bool on;
  const double e = group_eval(T, X, box, row, m, F, on);
  if (!on) return;
  const int kind = T.kind[m];
  for (int c = 0; c < kWidth; ++c)
    if (c == kind) energy[c] = e;
}

__global__ __launch_bounds__(kThreads) void group_energy_kernel(GroupTables T, double *__restrict__ partials, int nblocks, SideChunk B,
                                                                int rep0) {
#pragma clang fp contract(off)
  const int r = rep0 + blockIdx.y;
  const double box[3] = {B.box[blockIdx.y][0], B.box[blockIdx.y][1], B.box[blockIdx.y][2]};
  double energy[kWidth];
  group_energy_lane(T, T.centres + (size_t)r * T.ngroups * 3, box, r, energy);
  block_sums<kThreads / 64, Meet::Pairwise>(energy, partials + ((size_t)r * nblocks + blockIdx.x) * kWidth);
}

// one wave per replica (blockIdx.x counts from rep0): out[r][3] = the fold of the replica's partials
__global__ __launch_bounds__(64) void group_fold_kernel(const double *__restrict__ partials, int nblocks, double *__restrict__ out, int rep0) {
  const size_t r = (size_t)rep0 + blockIdx.x;
  double sum[kWidth];
  fold_rows(partials + r * nblocks * kWidth, nblocks, sum);
  if (threadIdx.x == 0)
    for (int c = 0; c < kWidth; ++c) out[kWidth * r + c] = sum[c];
}

// the energy kernel's walk with the table row on blockIdx.z; partials [R][R][nblocks][3], (configuration, row) outermost
__global__ __launch_bounds__(kThreads) void group_states_kernel(GroupTables T, double *__restrict__ partials, int nblocks, int nrep,
                                                                SideChunk B, int rep0) {
#pragma clang fp contract(off)
  const int i = rep0 + blockIdx.y, row = blockIdx.z;
  const double box[3] = {B.box[blockIdx.y][0], B.box[blockIdx.y][1], B.box[blockIdx.y][2]};
  double energy[kWidth];
  group_energy_lane(T, T.centres + (size_t)i * T.ngroups * 3, box, row, energy);
  block_sums<kThreads / 64, Meet::Pairwise>(energy, partials + (((size_t)i * nrep + row) * nblocks + blockIdx.x) * kWidth);
}

__global__ __launch_bounds__(64) void group_states_fold_kernel(const double *__restrict__ partials, int nblocks, double *__restrict__ out) {
  const size_t ik = blockIdx.x;
  double sum[kWidth];
  fold_rows(partials + ik * nblocks * kWidth, nblocks, sum);
  if (threadIdx.x == 0)
    for (int c = 0; c < kWidth; ++c) out[kWidth * ik + c] = sum[c];
}

template <typename R>
int launch_states(GroupState *S, const void *pos, const double *box_host, hipStream_t st) {
  const GroupTables T = S->tables();
  const size_t stride = (size_t)S->natoms * 3;
  for (int c0 = 0; c0 < S->nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, S->nrep - c0);
    const SideChunk B = side_chunk(nr, c0, pos, nullptr, box_host, stride * sizeof(R));
    hipLaunchKernelGGL(group_centre_kernel<R>, dim3((unsigned)S->ngroups, (unsigned)nr), dim3(kThreads), 0, st, T, B, c0);
    hipLaunchKernelGGL(group_states_kernel, dim3((unsigned)S->nblocks_m, (unsigned)nr, (unsigned)S->nrep), dim3(kThreads), 0, st, T,
                       S->cross_partials.as<double>(), S->nblocks_m, S->nrep, B, c0);
  }
  hipLaunchKernelGGL(group_states_fold_kernel, dim3((unsigned)(S->nrep * S->nrep)), dim3(64), 0, st, S->cross_partials.as<double>(),
                     S->nblocks_m, S->cross.as<double>());
  TMD_HIP(hipGetLastError());
  return 0;
}

// arguments as SideTerm::launch
template <typename R>
int launch(GroupState *S, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces, void *vel,
           const void *mass, double kick, double *out, hipStream_t st) {
  const GroupTables T = S->tables();
  const size_t stride = (size_t)S->natoms * 3;
  for (int c0 = 0; c0 < nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, nrep - c0);
    const SideChunk B = side_chunk(nr, c0, pos, pos_each, box_host, stride * sizeof(R));
    hipLaunchKernelGGL(group_centre_kernel<R>, dim3((unsigned)S->ngroups, (unsigned)nr), dim3(kThreads), 0, st, T, B, rep0 + c0);
    if (forces || vel)
      hipLaunchKernelGGL(group_force_kernel<R>, dim3((unsigned)S->nblocks_a, (unsigned)nr), dim3(kThreads), 0, st, T,
                         forces ? (R *)forces + c0 * stride : nullptr, vel ? (R *)vel + c0 * stride : nullptr, (const R *)mass, kick, B,
                         rep0 + c0);
    if (out)
      hipLaunchKernelGGL(group_energy_kernel, dim3((unsigned)S->nblocks_m, (unsigned)nr), dim3(kThreads), 0, st, T,
                         S->partials.as<double>(), S->nblocks_m, B, rep0 + c0);
  }
  if (out) hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)nrep), dim3(64), 0, st, S->partials.as<double>(), S->nblocks_m, out, rep0);
  TMD_HIP(hipGetLastError());
  return 0;
}

static_assert(kSideWidth[kSideGroups] == kWidth, "group_fold_kernel writes (distance, angle, dihedral) per replica");
GroupState *state_of(tmdhip_ctx *ctx) { return (GroupState *)ctx->side[kSideGroups].state; }

int launch_any(tmdhip_ctx *ctx, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces,
               void *vel, const void *mass, double kick, double *out, hipStream_t st) {
  GroupState *S = state_of(ctx);
  return ctx->d.dtype == TMDHIP_F32 ? launch<float>(S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st)
                                    : launch<double>(S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st);
}

// a group atom without mass has no acceleration: refused where masses are first seen (one read-back per mass array)
int check_masses(tmdhip_ctx *ctx, const char *, const double *, const void *mass_dev, hipStream_t st) {
  GroupState *S = state_of(ctx);
  if (!mass_dev || S->mass_checked == mass_dev) return 0;
  std::vector<char> host((size_t)ctx->real_size * S->natoms);
  TMD_HIP(hipMemcpyAsync(host.data(), mass_dev, host.size(), hipMemcpyDeviceToHost, st));
  TMD_HIP(hipStreamSynchronize(st));
  for (int32_t a : S->atom_h) {
    const double m = ctx->d.dtype == TMDHIP_F32 ? (double)((const float *)host.data())[a] : ((const double *)host.data())[a];
    if (!(m > 0.0)) return fail("group restraints: atom " + std::to_string(a) + " belongs to a group and has no mass");
  }
  S->mass_checked = mass_dev;
  return 0;
}

double *run_energy(tmdhip_ctx *ctx) { return state_of(ctx)->energy.as<double>(); }

void release(tmdhip_ctx *ctx) {
  GroupState *S = state_of(ctx);
  if (!S) return;
  S->release();
  delete S;
  ctx->side[kSideGroups] = SideTerm{};
}

template <typename T>
int upload(DevBuf &b, const T *src, size_t count) {
  TMD_TRY(b.ensure(std::max<size_t>(sizeof(T) * count, 16)));
  if (count) TMD_HIP(hipMemcpy(b.p, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

extern "C" {

int tmdhip_set_group_restraints(tmdhip_ctx *ctx, const tmdhip_group_restraint_desc *desc) {
  const std::string who = "tmdhip_set_group_restraints: ";
  if (!ctx || !desc) return fail(who + "null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_group_restraint_desc)) return fail(who + "tmdhip_group_restraint_desc size mismatch (ABI)");
  if (!desc->enable || desc->nrestraints == 0) {
    TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the tables may still be in flight)
    release(ctx);
    return 0;
  }
  const int n = ctx->d.natoms, nrep = (int)ctx->rep.size();
  if (desc->nreplicas != nrep) return fail(who + "nreplicas must be the context's");
  if (ctx->nactive < n) return fail(who + "not for a context with passive atoms (a brick of the domain decomposition)");
  const int G = desc->ngroups, M = desc->nrestraints;
  const std::string why = group_validate(n, nrep, G, desc->group_off_host, desc->member_atom_host, desc->member_weight_host, M,
                                         desc->kind_host, desc->groups_host, desc->target_host, desc->k_host, desc->flat_host);
  if (!why.empty()) return fail(who + why);
  if (ctx->vsites) {
    const VsiteState *V = (const VsiteState *)ctx->vsites;
    for (int32_t m = 0; m < desc->group_off_host[G]; ++m)
      if (std::find(V->site_h.begin(), V->site_h.end(), desc->member_atom_host[m]) != V->site_h.end())
        return fail(who + "atom " + std::to_string(desc->member_atom_host[m]) + " is a virtual site (name its parents)");
  }
  std::vector<double> w;
  group_normalise(G, desc->group_off_host, desc->member_weight_host, w);
  std::vector<int32_t> use_off, atoms, mem_off;
  std::vector<GroupUse> use;
  std::vector<GroupMember> mem;
  group_build_csr(G, desc->group_off_host, desc->member_atom_host, M, desc->kind_host, desc->groups_host, use_off, use, atoms, mem_off, mem);
  TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the old tables may still be in flight)
  GroupState *S = state_of(ctx);
  if (!S) ctx->side[kSideGroups] = SideTerm{S = new GroupState, "group restraints need", launch_any, check_masses, run_energy, release};
  const bool same_atoms = S->atom_h == atoms;
  S->nrep = nrep;
  S->natoms = n;
  S->ngroups = G;
  S->nrest = M;
  S->nrows = (int)atoms.size();
  S->nblocks_a = (S->nrows + kThreads - 1) / kThreads;
  S->nblocks_m = (M + kThreads - 1) / kThreads;
  S->atom_h = atoms;
  if (!same_atoms) S->mass_checked = nullptr;
  const size_t nm = (size_t)desc->group_off_host[G], rm = (size_t)nrep * M;
  int rc = upload(S->group_off, desc->group_off_host, (size_t)G + 1);
  if (rc == 0) rc = upload(S->member_atom, desc->member_atom_host, nm);
  if (rc == 0) rc = upload(S->member_w, w.data(), nm);
  if (rc == 0) rc = upload(S->kind, desc->kind_host, (size_t)M);
  if (rc == 0) rc = upload(S->groups, desc->groups_host, 4 * (size_t)M);
  if (rc == 0) rc = upload(S->use_off, use_off.data(), use_off.size());
  if (rc == 0) rc = upload(S->use, use.data(), use.size());
  if (rc == 0) rc = upload(S->atom, atoms.data(), atoms.size());
  if (rc == 0) rc = upload(S->mem_off, mem_off.data(), mem_off.size());
  if (rc == 0) rc = upload(S->mem, mem.data(), mem.size());
  if (rc == 0) rc = upload(S->target, desc->target_host, rm);
  if (rc == 0) rc = upload(S->k, desc->k_host, rm);
  if (rc == 0) rc = upload(S->flat, desc->flat_host, rm);
  if (rc == 0) rc = S->centres.ensure(sizeof(double) * 3 * (size_t)nrep * G);
  if (rc == 0) rc = S->partials.ensure(sizeof(double) * kWidth * (size_t)nrep * S->nblocks_m);
  if (rc == 0 && S->energy.bytes < sizeof(double) * kWidth * (size_t)nrep) {
    rc = S->energy.ensure(sizeof(double) * kWidth * (size_t)nrep);
    if (rc == 0 && hipMemset(S->energy.p, 0, S->energy.bytes) != hipSuccess) rc = fail(who + "hipMemset failed");
  }
  if (rc != 0) {
    release(ctx);
    return rc;
  }
  TMD_HIP(hipDeviceSynchronize());
  return 0;
}

int tmdhip_group_restraint_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev,
                                 const void *mass_dev, double kick, double *energies_dev, void *stream) {
  return side_apply(ctx, kSideGroups, "tmdhip_group_restraint_apply", pos_dev, box_host, forces_dev, vel_dev, mass_dev, kick,
                    energies_dev, stream);
}

int tmdhip_group_restraint_energy(tmdhip_ctx *ctx, double *out_host, void *stream) {
  return side_energy(ctx, kSideGroups, "tmdhip_group_restraint_energy", out_host, stream);
}

int tmdhip_group_restraint_states(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, double *out_host, void *stream) {
  if (!ctx || !pos_dev || !box_host || !out_host) return fail("tmdhip_group_restraint_states: null argument");
  GroupState *S = state_of(ctx);
  const size_t nrep = ctx->rep.size(), count = kWidth * nrep * nrep;
  if (!S) {
    std::fill(out_host, out_host + count, 0.0);
    return 0;
  }
  if (nrep > 65535) return fail("tmdhip_group_restraint_states: at most 65535 replicas (the table row is a grid axis)");
  hipStream_t st = (hipStream_t)stream;
  // (a buffer that grows is freed: nothing of an earlier call is in flight, every call ends with a synchronisation)
  TMD_TRY(S->cross_partials.ensure(sizeof(double) * count * S->nblocks_m));
  TMD_TRY(S->cross.ensure(sizeof(double) * count));
  TMD_TRY(ctx->d.dtype == TMDHIP_F32 ? launch_states<float>(S, pos_dev, box_host, st) : launch_states<double>(S, pos_dev, box_host, st));
  TMD_HIP(hipMemcpyAsync(out_host, S->cross.p, sizeof(double) * count, hipMemcpyDeviceToHost, st));
  TMD_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
