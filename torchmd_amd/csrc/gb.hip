// Generalized-Born implicit solvent (OBC2 + the ACE-type surface-area term) for open-boundary contexts, gfx950
// (tmdhip_set_gb, tmdhip_gb_apply, tmdhip_gb_energy, tmdhip_gb_born_radii; the arithmetic: gb_math.h).
//
// Three dependent O(N^2) pair passes, each followed by a per-atom close:
//   pass 1  I_i = (1/2) sum_j t(i <- j)                       close: B_i, c_i
//   pass 2  sum_j G_ij, sum_j h_ij B_j, sum_j g_ij (x_j - x_i)   close: E_SA,i, b_i = dE/dI_i
//   pass 3  sum_j [b_i t3(i <- j) + b_j t3(j <- i)] (x_i - x_j) / r   close: F_i into forces and / or velocities
// The pair kernels have one shape: ONE WAVE per block, one lane per atom i, grid (ceil(N/64), nsplit, replicas of the launch).
// Block (x, y) walks atoms 64 x .. against the j range [y jchunk, (y + 1) jchunk), which streams through LDS in tiles of 64
// records (x, y, z and what the pass needs of j); every lane reads record k of the tile at the same time (an LDS broadcast).
// Every pair is visited from both sides: twice the arithmetic, but every (i, split) has one writer, the closes add the splits
// in index order, and there is no floating-point atomic anywhere: two calls on the same state return the same bits.
// d, r and the per-pair functions are formed in the context's precision (fp32: full-precision expf / logf / sqrtf, IEEE
// division); every sum over j, the closes and the energies are double.  Energies: fixed-order sum (reduce.h) of one-wave blocks,
// then one wave per replica folds the partials.
// nsplit: about 2048 waves per launch (two per SIMD of the 256 CUs), jchunk a multiple of the tile; TMDHIP_GB_NSPLIT (read by
// tmdhip_set_gb) forces the split (tests).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "engine.h"
#include "gb_math.h"

using namespace tmd;

namespace {

constexpr int kTile = 64;
constexpr int kWantWaves = 2048;

struct ChunkPos {  // where the positions of each replica of a launch live (real [N][3])
  const void *pos[kSideChunk];
};

struct GbState {
  int nrep = 0, natoms = 0, nb = 0, nsplit = 1, jchunk = kTile;
  double p = 0;  // -(1/eps_in - 1/eps_out): the charges on the device carry sqrt(k_e) each
  DevBuf rho, sig;     // real [N]
  DevBuf radius, sa;   // double [N]: r_i, 4 pi gamma (r_i + r_probe)^2
  DevBuf part1;        // double [R][nsplit][N]
  DevBuf part2;        // double [R][nsplit][N][4]: b, direct force
  DevBuf part3;        // double [R][nsplit][N][3]
  DevBuf born, cfac;   // double [R][N]: B_i, c_i of the last evaluation
  DevBuf born_r, b_r;  // real [R][N]: B_i, b_i as the pair passes read them
  DevBuf epart;        // double [R][nsplit nb + nb]: the pair blocks' sums of G, then the close blocks' sums of E_SA
  DevBuf energy;       // double [R][2]: (GB, SA) of the last tmdhip_md_run
  void release() {
    for (DevBuf *b : {&rho, &sig, &radius, &sa, &part1, &part2, &part3, &born, &cfac, &born_r, &b_r, &epart, &energy}) b->release();
  }
};

template <typename R>
struct Tile4 {
  R x, y, z, w;
};

// the lane's own atom (clamped to the last atom for the idle lanes of the last block: they compute and store nothing)
#define GB_PROLOGUE                                                                       \
  const int lane = threadIdx.x, i = blockIdx.x * kTile + lane, ic = i < n ? i : n - 1;   \
  const R *__restrict__ pos = (const R *)P.pos[blockIdx.z];                               \
  const R xi = pos[3 * ic], yi = pos[3 * ic + 1], zi = pos[3 * ic + 2];                   \
  const int j0 = blockIdx.y * jchunk, j1 = min(n, j0 + jchunk);                           \
  const size_t row = ((size_t)(rep0 + blockIdx.z) * gridDim.y + blockIdx.y) * n + ic;     \
  const size_t arow = (size_t)(rep0 + blockIdx.z) * n

template <typename R>
__global__ __launch_bounds__(kTile) void gb_born_kernel(int n, int jchunk, ChunkPos P, int rep0, const R *__restrict__ rho,
                                                        const R *__restrict__ sig, double *__restrict__ part1) {
  GB_PROLOGUE;
  (void)arow;
  __shared__ Tile4<R> tile[kTile];
  const R rho_i = rho[ic];
  double acc = 0.0;
  for (int jt = j0; jt < j1; jt += kTile) {
    __syncthreads();
    const int j = jt + lane;
    if (j < j1) tile[lane] = {pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], sig[j]};
    __syncthreads();
    const int cnt = min(kTile, j1 - jt);
    for (int k = 0; k < cnt; ++k) {
      const Tile4<R> t = tile[k];
      if (jt + k == i) continue;
      const R dx = t.x - xi, dy = t.y - yi, dz = t.z - zi;
      const R r = gb_sqrt((dx * dx + dy * dy) + dz * dz);
      acc += (double)gb_pair_t(r, rho_i, t.w);
    }
  }
  if (i < n) part1[row] = acc;
}

template <typename R>
__global__ __launch_bounds__(kTile) void gb_energy_kernel(int n, int jchunk, ChunkPos P, int rep0, R p, const R *__restrict__ qs,
                                                          const R *__restrict__ born_r, double *__restrict__ part2,
                                                          double *__restrict__ epart, int estride) {
  GB_PROLOGUE;
  __shared__ Tile4<R> tile[kTile];
  __shared__ R tileB[kTile];
  const R pq = p * qs[ic], Bi = born_r[arow + ic];
  double eacc = 0.0, bacc = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
  for (int jt = j0; jt < j1; jt += kTile) {
    __syncthreads();
    const int j = jt + lane;
    if (j < j1) {
      tile[lane] = {pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], qs[j]};
      tileB[lane] = born_r[arow + j];
    }
    __syncthreads();
    const int cnt = min(kTile, j1 - jt);
    for (int k = 0; k < cnt; ++k) {  // (j = i included: r = 0 is the self term, and its force is g * 0)
      const Tile4<R> t = tile[k];
      const R Bj = tileB[k];
      const R dx = t.x - xi, dy = t.y - yi, dz = t.z - zi;
      const GbPair<R> o = gb_pair_energy((dx * dx + dy * dy) + dz * dz, pq * t.w, Bi, Bj);
      eacc += (double)o.G;
      bacc += (double)(o.h * Bj);
      fx += (double)(o.g * dx);
      fy += (double)(o.g * dy);
      fz += (double)(o.g * dz);
    }
  }
  if (i < n) {
    double *o = part2 + 4 * row;
    o[0] = bacc, o[1] = fx, o[2] = fy, o[3] = fz;
  }
  const double e[1] = {i < n ? eacc : 0.0};
  block_sums<1, Meet::Pairwise>(e, epart + (size_t)(rep0 + blockIdx.z) * estride + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

template <typename R>
__global__ __launch_bounds__(kTile) void gb_chain_kernel(int n, int jchunk, ChunkPos P, int rep0, const R *__restrict__ rho,
                                                         const R *__restrict__ sig, const R *__restrict__ b_r,
                                                         double *__restrict__ part3) {
  GB_PROLOGUE;
  __shared__ Tile4<R> tile[kTile];
  __shared__ R tileRho[kTile], tileb[kTile];
  const R rho_i = rho[ic], sig_i = sig[ic], bi = b_r[arow + ic];
  double fx = 0.0, fy = 0.0, fz = 0.0;
  for (int jt = j0; jt < j1; jt += kTile) {
    __syncthreads();
    const int j = jt + lane;
    if (j < j1) {
      tile[lane] = {pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], sig[j]};
      tileRho[lane] = rho[j];
      tileb[lane] = b_r[arow + j];
    }
    __syncthreads();
    const int cnt = min(kTile, j1 - jt);
    for (int k = 0; k < cnt; ++k) {
      const Tile4<R> t = tile[k];
      if (jt + k == i) continue;
      const R dx = t.x - xi, dy = t.y - yi, dz = t.z - zi;
      const R r = gb_sqrt((dx * dx + dy * dy) + dz * dz);
      // (x_i - x_j) / r = -d / r
      const R s = -(bi * gb_pair_t3(r, rho_i, t.w) + tileb[k] * gb_pair_t3(r, tileRho[k], sig_i)) / r;
      fx += (double)(s * dx);
      fy += (double)(s * dy);
      fz += (double)(s * dz);
    }
  }
  if (i < n) {
    double *o = part3 + 3 * row;
    o[0] = fx, o[1] = fy, o[2] = fz;
  }
}

// ---- the per-atom closes: one wave per block, grid (ceil(N/64), replicas of the launch); the splits are added in index order ----
template <typename R>
__global__ __launch_bounds__(kTile) void gb_close_born_kernel(int n, int nsplit, int rep0, const double *__restrict__ part1,
                                                              const double *__restrict__ radius, double *__restrict__ born,
                                                              double *__restrict__ cfac, R *__restrict__ born_r) {
  const int i = blockIdx.x * kTile + threadIdx.x, r = rep0 + blockIdx.y;
  if (i >= n) return;
  double sum = 0.0;
  for (int s = 0; s < nsplit; ++s) sum += part1[((size_t)r * nsplit + s) * n + i];
  double B, c;
  gb_close_born(0.5 * sum, radius[i], B, c);
  born[(size_t)r * n + i] = B;
  cfac[(size_t)r * n + i] = c;
  born_r[(size_t)r * n + i] = (R)B;
}

template <typename R>
__global__ __launch_bounds__(kTile) void gb_close_chain_kernel(int n, int nsplit, int rep0, const double *__restrict__ part2,
                                                               const double *__restrict__ radius, const double *__restrict__ sa,
                                                               const double *__restrict__ born, const double *__restrict__ cfac,
                                                               R *__restrict__ b_r, double *__restrict__ epart, int estride, int eoff) {
  const int i = blockIdx.x * kTile + threadIdx.x, r = rep0 + blockIdx.y;
  double esa[1] = {0.0};
  if (i < n) {
    double sum = 0.0;
    for (int s = 0; s < nsplit; ++s) sum += part2[4 * (((size_t)r * nsplit + s) * n + i)];
    double b;
    esa[0] = gb_close_chain(sum, radius[i], sa[i], born[(size_t)r * n + i], cfac[(size_t)r * n + i], b);
    b_r[(size_t)r * n + i] = (R)b;
  }
  block_sums<1, Meet::Pairwise>(esa, epart + (size_t)r * estride + eoff + blockIdx.x);
}

// forces / vel: the rows of the launch's first replica (blockIdx.y counts from it)
template <typename R>
__global__ __launch_bounds__(kTile) void gb_close_force_kernel(int n, int nsplit, int rep0, const double *__restrict__ part2,
                                                               const double *__restrict__ part3, R *__restrict__ forces,
                                                               R *__restrict__ vel, const R *__restrict__ mass, double kick) {
  const int i = blockIdx.x * kTile + threadIdx.x, r = rep0 + blockIdx.y;
  if (i >= n) return;
  double f[3] = {0.0, 0.0, 0.0};
  for (int s = 0; s < nsplit; ++s) {
    const double *a = part2 + 4 * (((size_t)r * nsplit + s) * n + i);
    for (int c = 0; c < 3; ++c) f[c] += a[1 + c];
  }
  for (int s = 0; s < nsplit; ++s) {
    const double *a = part3 + 3 * (((size_t)r * nsplit + s) * n + i);
    for (int c = 0; c < 3; ++c) f[c] += a[c];
  }
  side_store(forces, vel, ((size_t)blockIdx.y * n + i) * 3, mass, i, kick, f);
}

// one wave per replica (blockIdx.x counts from rep0): out[r] = ((1/2) sum of the pair partials, sum of the SA partials)
__global__ __launch_bounds__(64) void gb_fold_kernel(const double *__restrict__ epart, int estride, int npair, double *__restrict__ out,
                                                     int rep0) {
#pragma clang fp contract(off)
  const int r = rep0 + blockIdx.x;
  const double *e = epart + (size_t)r * estride;
  double sg[1] = {0.0}, ss[1] = {0.0};
  fold_into(sg, e, npair);
  fold_into(ss, e + npair, estride - npair);
  sg[0] = wave_sum(sg[0]), ss[0] = wave_sum(ss[0]);
  if (threadIdx.x == 0) {
    out[2 * (size_t)r] = 0.5 * sg[0];
    out[2 * (size_t)r + 1] = ss[0];
  }
}

// replicas rep0 .. rep0 + nrep - 1; forces / vel point at the rows of replica rep0; the positions are [nrep][N][3] at `pos`, or,
// with `pos_each`, one array per replica; `out` (double [R][2], indexed by the replica's number) wants the energies
template <typename R>
int launch(tmdhip_ctx *ctx, GbState *S, int rep0, int nrep, const void *pos, const void *const *pos_each, void *forces, void *vel,
           const void *mass, double kick, double *out, hipStream_t st) {
  const int n = S->natoms, nb = S->nb, ns = S->nsplit, estride = ns * nb + nb;
  const size_t stride = (size_t)n * 3;
  const R *qs = ctx->qs.as<R>(), *rho = S->rho.as<R>(), *sig = S->sig.as<R>();
  for (int c0 = 0; c0 < nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, nrep - c0), r0 = rep0 + c0;
    ChunkPos P;
    for (int r = 0; r < kSideChunk; ++r) P.pos[r] = r < nr ? side_pos(pos, pos_each, c0 + r, stride * sizeof(R)) : nullptr;
    const dim3 pair((unsigned)nb, (unsigned)ns, (unsigned)nr), atom((unsigned)nb, (unsigned)nr), block(kTile);
    hipLaunchKernelGGL(gb_born_kernel<R>, pair, block, 0, st, n, S->jchunk, P, r0, rho, sig, S->part1.as<double>());
    hipLaunchKernelGGL(gb_close_born_kernel<R>, atom, block, 0, st, n, ns, r0, S->part1.as<double>(), S->radius.as<double>(),
                       S->born.as<double>(), S->cfac.as<double>(), S->born_r.as<R>());
    hipLaunchKernelGGL(gb_energy_kernel<R>, pair, block, 0, st, n, S->jchunk, P, r0, (R)S->p, qs, S->born_r.as<R>(),
                       S->part2.as<double>(), S->epart.as<double>(), estride);
    hipLaunchKernelGGL(gb_close_chain_kernel<R>, atom, block, 0, st, n, ns, r0, S->part2.as<double>(), S->radius.as<double>(),
                       S->sa.as<double>(), S->born.as<double>(), S->cfac.as<double>(), S->b_r.as<R>(), S->epart.as<double>(), estride,
                       ns * nb);
    if (forces || vel) {
      hipLaunchKernelGGL(gb_chain_kernel<R>, pair, block, 0, st, n, S->jchunk, P, r0, rho, sig, S->b_r.as<R>(), S->part3.as<double>());
      hipLaunchKernelGGL(gb_close_force_kernel<R>, atom, block, 0, st, n, ns, r0, S->part2.as<double>(), S->part3.as<double>(),
                         forces ? (R *)forces + c0 * stride : nullptr, vel ? (R *)vel + c0 * stride : nullptr, (const R *)mass, kick);
    }
  }
  if (out) hipLaunchKernelGGL(gb_fold_kernel, dim3((unsigned)nrep), dim3(64), 0, st, S->epart.as<double>(), estride, ns * nb, out, rep0);
  TMD_HIP(hipGetLastError());
  return 0;
}

static_assert(kSideWidth[kSideGb] == 2, "gb_fold_kernel writes (GB, SA) per replica");
GbState *state_of(tmdhip_ctx *ctx) { return (GbState *)ctx->side[kSideGb].state; }

// (no box: check_boxes has seen that every edge is zero)
int launch_any(tmdhip_ctx *ctx, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *, void *forces, void *vel,
               const void *mass, double kick, double *out, hipStream_t st) {
  GbState *S = state_of(ctx);
  // (what tmdhip_set_gb refused may have been switched on since)
  if (S->natoms != ctx->d.natoms || S->nrep != (int)ctx->rep.size() || ctx->nactive < ctx->d.natoms || ctx->vsites || ctx->pme)
    return fail("generalized Born: the context has changed since tmdhip_set_gb (atoms, passive atoms, virtual sites or PME)");
  return ctx->d.dtype == TMDHIP_F32 ? launch<float>(ctx, S, rep0, nrep, pos, pos_each, forces, vel, mass, kick, out, st)
                                    : launch<double>(ctx, S, rep0, nrep, pos, pos_each, forces, vel, mass, kick, out, st);
}

// open boundaries only: every edge of every replica's box is zero
int check_boxes(tmdhip_ctx *ctx, const char *who, const double *box_host, const void *, hipStream_t) {
  for (size_t k = 0; k < 3 * ctx->rep.size(); ++k)
    if (box_host[k] != 0.0) return fail(std::string(who) + ": the generalized-Born model needs open boundaries (every box edge 0)");
  return 0;
}

template <typename T>
int upload(DevBuf &b, const std::vector<T> &src) {
  TMD_TRY(b.ensure(std::max<size_t>(sizeof(T) * src.size(), 16)));
  TMD_HIP(hipMemcpy(b.p, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return 0;
}

double *run_energy(tmdhip_ctx *ctx) { return state_of(ctx)->energy.as<double>(); }

void release(tmdhip_ctx *ctx) {
  GbState *S = state_of(ctx);
  if (!S) return;
  S->release();
  delete S;
  ctx->side[kSideGb] = SideTerm{};
}

}  // namespace

extern "C" {

int tmdhip_set_gb(tmdhip_ctx *ctx, const tmdhip_gb_desc *desc) {
  if (!ctx || !desc) return fail("tmdhip_set_gb: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_gb_desc)) return fail("tmdhip_set_gb: tmdhip_gb_desc size mismatch (ABI)");
  if (!desc->enable) {
    TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the tables may still be in flight)
    release(ctx);
    return 0;
  }
  const int n = ctx->d.natoms, nrep = (int)ctx->rep.size();
  if (!desc->radii_host || !desc->scale_host) return fail("tmdhip_set_gb: null radii or scales");
  if (ctx->nactive < n) return fail("tmdhip_set_gb: not for a context with passive atoms (a brick of the domain decomposition)");
  if (ctx->vsites) return fail("tmdhip_set_gb: not for a context with virtual sites");
  if (ctx->pme) return fail("tmdhip_set_gb: not with PME (a periodic method; the model is for open boundaries)");
  if (ctx->d.rfa) return fail("tmdhip_set_gb: not with the reaction field, which already stands for the solvent");
  if (!(desc->solute_dielectric > 0.0) || !(desc->solvent_dielectric > 0.0) || !std::isfinite(desc->solute_dielectric) ||
      !std::isfinite(desc->solvent_dielectric))
    return fail("tmdhip_set_gb: the dielectric constants must be finite and positive");
  if (!(desc->surface_tension >= 0.0) || !std::isfinite(desc->surface_tension) || !(desc->probe_radius >= 0.0) ||
      !std::isfinite(desc->probe_radius))
    return fail("tmdhip_set_gb: the surface tension and the probe radius must be finite and not negative");
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(desc->radii_host[i]) || !(desc->radii_host[i] > kGbOffset))
      return fail("tmdhip_set_gb: the radius of atom " + std::to_string(i) + " must be finite and above 0.09");
    if (!std::isfinite(desc->scale_host[i]) || !(desc->scale_host[i] >= 0.0))
      return fail("tmdhip_set_gb: the scale of atom " + std::to_string(i) + " must be finite and not negative");
  }
  TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the old tables may still be in flight)
  GbState *S = state_of(ctx);
  if (!S) ctx->side[kSideGb] = SideTerm{S = new GbState, "the generalized-Born model needs", launch_any, check_boxes, run_energy, release};
  S->nrep = nrep;
  S->natoms = n;
  S->nb = (n + kTile - 1) / kTile;
  const char *forced = std::getenv("TMDHIP_GB_NSPLIT");
  const int want = forced && std::atoi(forced) > 0 ? std::atoi(forced) : kWantWaves / std::max(S->nb * nrep, 1);
  const int ns0 = std::max(1, std::min(want, S->nb));
  S->jchunk = ((n + ns0 - 1) / ns0 + kTile - 1) / kTile * kTile;
  S->nsplit = (n + S->jchunk - 1) / S->jchunk;
  S->p = -(1.0 / desc->solute_dielectric - 1.0 / desc->solvent_dielectric);
  const double pi = 3.14159265358979323846;
  std::vector<double> radius(n), sa(n), rho(n), sig(n);
  for (int i = 0; i < n; ++i) {
    radius[i] = desc->radii_host[i];
    rho[i] = radius[i] - kGbOffset;
    sig[i] = desc->scale_host[i] * rho[i];
    const double rp = radius[i] + desc->probe_radius;
    sa[i] = 4.0 * pi * desc->surface_tension * rp * rp;
  }
  int rc = upload(S->radius, radius);
  if (rc == 0) rc = upload(S->sa, sa);
  if (rc == 0 && ctx->d.dtype == TMDHIP_F32) {
    rc = upload(S->rho, std::vector<float>(rho.begin(), rho.end()));
    if (rc == 0) rc = upload(S->sig, std::vector<float>(sig.begin(), sig.end()));
  } else if (rc == 0) {
    rc = upload(S->rho, rho);
    if (rc == 0) rc = upload(S->sig, sig);
  }
  const size_t rn = (size_t)nrep * n, prn = rn * S->nsplit;
  if (rc == 0) rc = S->part1.ensure(sizeof(double) * prn);
  if (rc == 0) rc = S->part2.ensure(sizeof(double) * 4 * prn);
  if (rc == 0) rc = S->part3.ensure(sizeof(double) * 3 * prn);
  if (rc == 0) rc = S->born.ensure(sizeof(double) * rn);
  if (rc == 0) rc = S->cfac.ensure(sizeof(double) * rn);
  if (rc == 0) rc = S->born_r.ensure((size_t)ctx->real_size * rn);
  if (rc == 0) rc = S->b_r.ensure((size_t)ctx->real_size * rn);
  if (rc == 0) rc = S->epart.ensure(sizeof(double) * (size_t)nrep * (S->nsplit * S->nb + S->nb));
  if (rc == 0) rc = S->energy.ensure(sizeof(double) * kSideWidth[kSideGb] * (size_t)nrep);
  if (rc == 0 && hipMemset(S->energy.p, 0, S->energy.bytes) != hipSuccess) rc = fail("tmdhip_set_gb: hipMemset failed");
  if (rc == 0 && hipMemset(S->born.p, 0, S->born.bytes) != hipSuccess) rc = fail("tmdhip_set_gb: hipMemset failed");
  if (rc != 0) {
    release(ctx);
    return rc;
  }
  TMD_HIP(hipDeviceSynchronize());
  return 0;
}

int tmdhip_gb_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev, const void *mass_dev,
                    double kick, double *energies_dev, void *stream) {
  return side_apply(ctx, kSideGb, "tmdhip_gb_apply", pos_dev, box_host, forces_dev, vel_dev, mass_dev, kick, energies_dev, stream);
}

int tmdhip_gb_energy(tmdhip_ctx *ctx, double *out_host, void *stream) {
  return side_energy(ctx, kSideGb, "tmdhip_gb_energy", out_host, stream);
}

int tmdhip_gb_born_radii(tmdhip_ctx *ctx, double *out_host) {
  if (!ctx || !out_host) return fail("tmdhip_gb_born_radii: null argument");
  GbState *S = state_of(ctx);
  if (!S) return fail("tmdhip_gb_born_radii: the context has no generalized-Born state (tmdhip_set_gb)");
  TMD_HIP(hipDeviceSynchronize());
  TMD_HIP(hipMemcpy(out_host, S->born.p, sizeof(double) * (size_t)S->nrep * S->natoms, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
