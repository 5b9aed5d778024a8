// Alchemical decoupling of a solute S from its environment E with one coupling (lambda_vdw, lambda_elec) per replica, gfx950
// (tmdhip_set_alchemical, tmdhip_alchemical_apply, tmdhip_alchemical_energy, tmdhip_alchemical_states; the arithmetic:
// alchemy_math.h).
//
// The context itself holds the solute with charge 0 and an all-zero Lennard-Jones class, so its own pair kernels return exactly
// 0 for every pair that names a solute atom.  What they leave out is added here, as an impulse between the launches of
// tmdhip_md_run or on top of an evaluation:
//   cross   every pair (i in S, j in E) inside the engine's cutoff (min_image, norm2, r2max of pair_math.h): soft-core
//           Lennard-Jones and lambda_elec times the engine's electrostatics, with dU/dlambda in the same pass
//   intra   the non-excluded S-S pairs at full strength and the charge part of the solute's 1-4 pairs
// Kernels (one wave per block, blockIdx.z or .y = replica of the launch, kSideChunk replicas per launch):
//   bounds  one wave per replica: a sphere (centre, radius) around the solute, for the early-outs
//   env     lanes are the atoms of the system; the solute's records stream from LDS as broadcasts; a lane that stands for an
//           environment atom sums its own force in double and is its only writer.  A wave none of whose atoms lies within
//           radius + cutoff of the centre stops before the loop.  The energies and derivatives are counted here only.
//   solute  lanes are solute atoms, grid.y splits the system into chunks that stream through LDS; one partial force per
//           (atom, split).  A tile with no atom inside the sphere is skipped.
//   close   one wave per solute atom: the lanes share its partials and the entries of its intra row (both ends of every pair
//           are evaluated, the energy is counted by the lower index), a butterfly adds them in one fixed order, and lane 0 is
//           the only writer of the atom.  (One thread per atom, restraint.hip's scheme, is a chain of dependent loads as long
//           as the split count: 267 us per application on the 98 304-atom box with a 30-atom solute, against 6 us.)
//   fold    one wave per replica folds the blocks' partial sums: fixed-order sum (reduce.h) of one-wave blocks
// env and close serve whatever pointer is not null, like restraint_kernel: forces += F, vel += kick F / m (rows with m <= 0 are
// left alone), or both.  Rows of environment atoms with no solute atom inside the cutoff are never written.  Distances and pair
// functions are in the context's precision; every sum over partners, the energies and the derivatives are double.  There is no
// floating-point atomic: two calls on the same state give the same bits.
// The bounds launch and the early-outs are off by default: measured at solutes of 30 and 300 atoms they cost a few us a step more
// than they return.  TMDHIP_ALCHEMY_SPHERE=1 (read by tmdhip_set_alchemical) switches them on (timing, tests); TMDHIP_ALCHEMY_NSPLIT forces the
// split of the solute pass (tests).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "alchemy_math.h"
#include "engine.h"

using namespace tmd;

namespace {

constexpr int kTile = 64;
constexpr int kWantWaves = 2048;  // of the solute pass: a wave walks its chunk serially, so short chunks (measured: DESIGN §22)
constexpr int kMaxStates = 32;    // of one tmdhip_alchemical_states call

struct ChunkArgs {  // per replica of a launch: box, 1 / box (0: no image along the axis), its coupling, where its positions live
  double box[kSideChunk][3], invbox[kSideChunk][3];
  double lam_v[kSideChunk], lam_e[kSideChunk];
  const void *pos[kSideChunk];
};

struct StateArgs {
  int K;
  double lam_v[kMaxStates], lam_e[kMaxStates];
};

template <typename R>
struct Tables {
  int n, ns, ntypes;
  const int32_t *slot;   // [N]: the atom's row among the solute atoms, -1 for the environment
  const int32_t *types;  // [N]: the context's classes (the null class for the solute)
  const R *qs;           // [N]: the context's scaled charges (0 for the solute)
  const typename Vec<R>::T2 *tab;
  const int32_t *atoms;  // [ns] ascending
  const R *sq;           // [ns] the solute's scaled charges
  const int32_t *scls;   // [ns] its classes
};

struct AlchState {
  int nrep = 0, natoms = 0, ns = 0, nbA = 0, nbS = 0, nsplit = 1, jchunk = kTile;
  bool sphere = true;
  double alpha = 0;
  std::vector<double> lam_v, lam_e;
  // what the tables were built from: a call that changes nothing but the couplings updates lam_v / lam_e alone
  std::vector<int32_t> atoms_h, cls_h, pair14_h;
  std::vector<double> qs_h, scee_h;
  DevBuf slot, atoms, sq, scls, off, ent;
  DevBuf part;    // double [R][ns][nsplit][3]
  DevBuf epartA;  // double [R][nbA][3]: sums of U_lj, qq g, dU/dlv of the env blocks
  DevBuf epartC;  // double [R][ns]: the intra energy of the close waves
  DevBuf sph;     // double [R][4]
  DevBuf spart;   // double [R][nbA][kMaxStates + 1]
  DevBuf sout;    // double [R][kMaxStates]
  DevBuf energy;  // double [R][5] of the last tmdhip_md_run
  void release() {
    for (DevBuf *b : {&slot, &atoms, &sq, &scls, &off, &ent, &part, &epartA, &epartC, &sph, &spart, &sout, &energy}) b->release();
  }
};

template <typename R>
struct Rec4 {
  R x, y, z, q;
};

template <typename R>
__device__ __forceinline__ R image_r2(R dx, R dy, R dz, const R (&box)[3], const R (&inv)[3], R &ox, R &oy, R &oz) {
  ox = min_image(dx, box[0], inv[0]);
  oy = min_image(dy, box[1], inv[1]);
  oz = min_image(dz, box[2], inv[2]);
  return norm2(ox, oy, oz);
}

#define ALCH_BOX(z)                                                                                   \
  const R box[3] = {(R)P.box[z][0], (R)P.box[z][1], (R)P.box[z][2]};                                  \
  const R inv[3] = {(R)P.invbox[z][0], (R)P.invbox[z][1], (R)P.invbox[z][2]}

// sph[r] = (centre, radius): the centre is the mean of the solute's minimum images around its first atom, the radius the
// largest distance of a solute atom from it.  One wave per replica of the launch.
template <typename R>
__global__ __launch_bounds__(kTile) void alch_bounds_kernel(Tables<R> T, ChunkArgs P, int rep0, double *__restrict__ sph) {
  ALCH_BOX(blockIdx.x);
  const R *__restrict__ pos = (const R *)P.pos[blockIdx.x];
  const int a0 = T.atoms[0];
  const R x0 = pos[3 * a0], y0 = pos[3 * a0 + 1], z0 = pos[3 * a0 + 2];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int t = threadIdx.x; t < T.ns; t += kTile) {
    const int a = T.atoms[t];
    R dx, dy, dz;
    image_r2<R>(pos[3 * a] - x0, pos[3 * a + 1] - y0, pos[3 * a + 2] - z0, box, inv, dx, dy, dz);
    sx += (double)dx, sy += (double)dy, sz += (double)dz;
  }
  const R cx = x0 + (R)(wave_sum(sx) / T.ns), cy = y0 + (R)(wave_sum(sy) / T.ns), cz = z0 + (R)(wave_sum(sz) / T.ns);
  double r2 = 0.0;
  for (int t = threadIdx.x; t < T.ns; t += kTile) {
    const int a = T.atoms[t];
    R dx, dy, dz;
    r2 = fmax(r2, (double)image_r2<R>(pos[3 * a] - cx, pos[3 * a + 1] - cy, pos[3 * a + 2] - cz, box, inv, dx, dy, dz));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r2 = fmax(r2, __shfl_xor(r2, o, 64));
  if (threadIdx.x == 0) {
    double *o = sph + 4 * (size_t)(rep0 + blockIdx.x);
    o[0] = (double)cx, o[1] = (double)cy, o[2] = (double)cz, o[3] = sqrt(r2);
  }
}

// (radius + cutoff)^2 with room for the rounding of either side: a pair inside the cutoff is never on the far side of it
template <typename R>
__device__ __forceinline__ R sphere_reach2(const double *s, R r2max) {
  const double reach = (s[3] + sqrt((double)r2max)) * 1.001 + 1e-3;
  return (R)(reach * reach);
}

// Lanes are the atoms of the system (grid.x = ceil(N / 64), grid.y = replicas of the launch).
template <typename R>
__global__ __launch_bounds__(kTile) void alch_env_kernel(Tables<R> T, AlchConsts<R> c, ChunkArgs P, int rep0, const double *__restrict__ sph,
                                                         R *__restrict__ forces, R *__restrict__ vel, const R *__restrict__ mass,
                                                         double kick, double *__restrict__ epart) {
  ALCH_BOX(blockIdx.y);
  const int lane = threadIdx.x, i = blockIdx.x * kTile + lane, ic = i < T.n ? i : T.n - 1, r = rep0 + blockIdx.y;
  const R *__restrict__ pos = (const R *)P.pos[blockIdx.y];
  const bool mine = i < T.n && T.slot[ic] < 0;
  const R xi = pos[3 * ic], yi = pos[3 * ic + 1], zi = pos[3 * ic + 2], qi = T.qs[ic];
  const int ti = T.types[ic] * T.ntypes;
  const R lv = (R)P.lam_v[blockIdx.y], le = (R)P.lam_e[blockIdx.y];
  double *eo = epart ? epart + 3 * ((size_t)r * gridDim.x + blockIdx.x) : nullptr;
  if (sph) {
    const double *s = sph + 4 * (size_t)r;
    R dx, dy, dz;
    const bool near = mine && image_r2<R>(xi - (R)s[0], yi - (R)s[1], zi - (R)s[2], box, inv, dx, dy, dz) <= sphere_reach2<R>(s, c.r2max);
    if (!__any(near)) {
      if (eo && lane < 3) eo[lane] = 0.0;
      return;
    }
  }
  __shared__ Rec4<R> tile[kTile];
  __shared__ int tcls[kTile];
  double fx = 0.0, fy = 0.0, fz = 0.0, slj = 0.0, sgel = 0.0, sdv = 0.0;
  bool touched = false;
  for (int t0 = 0; t0 < T.ns; t0 += kTile) {
    __syncthreads();
    if (t0 + lane < T.ns) {
      const int a = T.atoms[t0 + lane];
      tile[lane] = {pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], T.sq[t0 + lane]};
      tcls[lane] = T.scls[t0 + lane];
    }
    __syncthreads();
    const int cnt = min(kTile, T.ns - t0);
    for (int k = 0; k < cnt; ++k) {
      const Rec4<R> t = tile[k];
      R dx, dy, dz;
      const R r2 = image_r2<R>(xi - t.x, yi - t.y, zi - t.z, box, inv, dx, dy, dz);
      if (!(mine && r2 <= c.r2max)) continue;
      const typename Vec<R>::T2 ab = T.tab[ti + tcls[k]];
      const AlchPair<R> o = alch_pair<R>(c, r2, qi * t.q, ab.x, ab.y, lv, le);
      touched = true;
      fx -= (double)(dx * o.fs), fy -= (double)(dy * o.fs), fz -= (double)(dz * o.fs);
      slj += (double)o.ulj, sgel += (double)o.gel, sdv += (double)o.dv;
    }
  }
  if (touched) {
    const double f[3] = {fx, fy, fz};
    side_store(forces, vel, ((size_t)blockIdx.y * T.n + i) * 3, mass, i, kick, f);
  }
  if (!eo) return;  // (uniform: a kernel argument)
  const double e[3] = {slj, sgel, sdv};
  block_sums<1, Meet::Pairwise>(e, eo);
}

// Lanes are solute atoms (grid.x = ceil(ns / 64), grid.y = splits of the system, grid.z = replicas of the launch).
template <typename R>
__global__ __launch_bounds__(kTile) void alch_solute_kernel(Tables<R> T, AlchConsts<R> c, ChunkArgs P, int rep0, int jchunk,
                                                            const double *__restrict__ sph, double *__restrict__ part) {
  ALCH_BOX(blockIdx.z);
  const int lane = threadIdx.x, t = blockIdx.x * kTile + lane, tc = t < T.ns ? t : T.ns - 1, r = rep0 + blockIdx.z;
  const R *__restrict__ pos = (const R *)P.pos[blockIdx.z];
  const int a = T.atoms[tc], cls = T.scls[tc];
  const R xi = pos[3 * a], yi = pos[3 * a + 1], zi = pos[3 * a + 2], qi = T.sq[tc];
  const R lv = (R)P.lam_v[blockIdx.z], le = (R)P.lam_e[blockIdx.z];
  const int j0 = blockIdx.y * jchunk, j1 = min(T.n, j0 + jchunk);
  const double *s = sph ? sph + 4 * (size_t)r : nullptr;
  const R reach2 = s ? sphere_reach2<R>(s, c.r2max) : R(0);
  __shared__ Rec4<R> tile[kTile];
  __shared__ int ttype[kTile];  // class row offset of the tile's atom, -1: not an environment atom
  double fx = 0.0, fy = 0.0, fz = 0.0;
  for (int jt = j0; jt < j1; jt += kTile) {
    __syncthreads();
    const int j = jt + lane;
    bool near = false;
    if (j < j1) {
      const Rec4<R> rec = {pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], T.qs[j]};
      const bool env = T.slot[j] < 0;
      tile[lane] = rec;
      ttype[lane] = env ? T.types[j] * T.ntypes : -1;
      R dx, dy, dz;
      near = env && (!s || image_r2<R>(rec.x - (R)s[0], rec.y - (R)s[1], rec.z - (R)s[2], box, inv, dx, dy, dz) <= reach2);
    }
    __syncthreads();
    if (!__any(near)) continue;
    const int cnt = min(kTile, j1 - jt);
    for (int k = 0; k < cnt; ++k) {
      const int tj = ttype[k];
      if (tj < 0) continue;
      const Rec4<R> e = tile[k];
      R dx, dy, dz;
      const R r2 = image_r2<R>(xi - e.x, yi - e.y, zi - e.z, box, inv, dx, dy, dz);
      if (!(r2 <= c.r2max)) continue;
      const typename Vec<R>::T2 ab = T.tab[tj + cls];
      const AlchPair<R> o = alch_pair<R>(c, r2, e.q * qi, ab.x, ab.y, lv, le);
      fx -= (double)(dx * o.fs), fy -= (double)(dy * o.fs), fz -= (double)(dz * o.fs);
    }
  }
  if (t < T.ns) {
    double *o = part + 3 * (((size_t)r * T.ns + t) * gridDim.y + blockIdx.y);
    o[0] = fx, o[1] = fy, o[2] = fz;
  }
}

// One wave per solute atom (grid.x = ns, grid.y = replicas of the launch): lane l adds the atom's partials l, l + 64, ... and
// walks the entries l, l + 64, ... of its intra row, the xor butterfly adds the lanes in one fixed order, lane 0 stores.
template <typename R>
__global__ __launch_bounds__(kTile) void alch_close_kernel(Tables<R> T, AlchConsts<R> c, ChunkArgs P, int rep0, int nsplit,
                                                           const double *__restrict__ part, const int32_t *__restrict__ off,
                                                           const AlchEntry *__restrict__ ent, R *__restrict__ forces,
                                                           R *__restrict__ vel, const R *__restrict__ mass, double kick,
                                                           double *__restrict__ epart) {
  ALCH_BOX(blockIdx.y);
  const int t = blockIdx.x, lane = threadIdx.x, r = rep0 + blockIdx.y;
  const R *__restrict__ pos = (const R *)P.pos[blockIdx.y];
  const int a = T.atoms[t];
  double f[3] = {0.0, 0.0, 0.0}, e_intra = 0.0;
  const double *p = part + 3 * ((size_t)r * T.ns + t) * nsplit;
  for (int s = lane; s < nsplit; s += kTile) {
    f[0] += p[3 * s], f[1] += p[3 * s + 1], f[2] += p[3 * s + 2];
  }
  for (int e = off[t] + lane; e < off[t + 1]; e += kTile) {
    const AlchEntry en = ent[e];
    const int b = en.partner, lo = a < b ? a : b, hi = a < b ? b : a;
    R dx, dy, dz;
    const R r2 = image_r2<R>(pos[3 * lo] - pos[3 * hi], pos[3 * lo + 1] - pos[3 * hi + 1], pos[3 * lo + 2] - pos[3 * hi + 2], box, inv,
                             dx, dy, dz);
    R fs, en_pair;
    if (en.kind == 0) {
      if (!(r2 <= c.r2max)) continue;
      const AlchPair<R> o = alch_pair<R>(c, r2, (R)en.qq, (R)en.A, (R)en.B, R(1), R(1));
      fs = o.fs, en_pair = o.ulj + o.gel;
    } else {
      en_pair = alch_pair14<R>(r2, (R)en.qq, (R)en.scee, fs);
    }
    if (a < b) e_intra += (double)en_pair;
    const R sgn = a < b ? R(-1) : R(1);  // the force on the lower atom is -d fs
    f[0] += (double)(sgn * dx * fs), f[1] += (double)(sgn * dy * fs), f[2] += (double)(sgn * dz * fs);
  }
  f[0] = wave_sum(f[0]), f[1] = wave_sum(f[1]), f[2] = wave_sum(f[2]);
  e_intra = wave_sum(e_intra);
  if (lane != 0) return;
  side_store(forces, vel, ((size_t)blockIdx.y * T.n + a) * 3, mass, a, kick, f);
  if (epart) epart[(size_t)r * gridDim.x + t] = e_intra;
}

// one wave per replica of the launch: out[r] = (cross LJ, cross el, intra, dU/dlv, dU/dle)
__global__ __launch_bounds__(64) void alch_fold_kernel(const double *__restrict__ epartA, int nbA, const double *__restrict__ epartC, int nbS,
                                                       ChunkArgs P, int rep0, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int r = rep0 + blockIdx.x;
  double x[3] = {0.0, 0.0, 0.0}, e[1] = {0.0};  // cross: LJ, qq g, dU/dlv; intra
  fold_into(x, epartA + 3 * (size_t)r * nbA, nbA);
  fold_into(e, epartC + (size_t)r * nbS, nbS);
  x[0] = wave_sum(x[0]), x[1] = wave_sum(x[1]), x[2] = wave_sum(x[2]), e[0] = wave_sum(e[0]);
  if (threadIdx.x == 0) {
    double *o = out + 5 * (size_t)r;
    o[0] = x[0], o[1] = P.lam_e[blockIdx.x] * x[1], o[2] = e[0], o[3] = x[2], o[4] = x[1];
  }
}

// The cross energy at K other couplings: the env kernel's walk with one accumulator per state.  spart[r][block][k < K] = sum of
// the Lennard-Jones energies at state k, [kMaxStates] = sum of qq g.
template <typename R>
__global__ __launch_bounds__(kTile) void alch_states_kernel(Tables<R> T, AlchConsts<R> c, ChunkArgs P, int rep0, StateArgs S,
                                                            const double *__restrict__ sph, double *__restrict__ spart) {
  ALCH_BOX(blockIdx.y);
  const int lane = threadIdx.x, i = blockIdx.x * kTile + lane, ic = i < T.n ? i : T.n - 1, r = rep0 + blockIdx.y;
  const R *__restrict__ pos = (const R *)P.pos[blockIdx.y];
  const bool mine = i < T.n && T.slot[ic] < 0;
  const R xi = pos[3 * ic], yi = pos[3 * ic + 1], zi = pos[3 * ic + 2], qi = T.qs[ic];
  const int ti = T.types[ic] * T.ntypes;
  double *so = spart + (kMaxStates + 1) * ((size_t)r * gridDim.x + blockIdx.x);
  if (sph) {
    const double *s = sph + 4 * (size_t)r;
    R dx, dy, dz;
    const bool near = mine && image_r2<R>(xi - (R)s[0], yi - (R)s[1], zi - (R)s[2], box, inv, dx, dy, dz) <= sphere_reach2<R>(s, c.r2max);
    if (!__any(near)) {
      if (lane <= kMaxStates) so[lane] = 0.0;
      return;
    }
  }
  __shared__ Rec4<R> tile[kTile];
  __shared__ int tcls[kTile];
  __shared__ R slv[kMaxStates];
  if (lane < kMaxStates) slv[lane] = lane < S.K ? (R)S.lam_v[lane] : R(0);
  double acc[kMaxStates], sgel = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxStates; ++k) acc[k] = 0.0;
  for (int t0 = 0; t0 < T.ns; t0 += kTile) {
    __syncthreads();
    if (t0 + lane < T.ns) {
      const int a = T.atoms[t0 + lane];
      tile[lane] = {pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], T.sq[t0 + lane]};
      tcls[lane] = T.scls[t0 + lane];
    }
    __syncthreads();
    const int cnt = min(kTile, T.ns - t0);
    for (int k = 0; k < cnt; ++k) {
      const Rec4<R> t = tile[k];
      R dx, dy, dz;
      const R r2 = image_r2<R>(xi - t.x, yi - t.y, zi - t.z, box, inv, dx, dy, dz);
      if (!(mine && r2 <= c.r2max)) continue;
      const typename Vec<R>::T2 ab = T.tab[ti + tcls[k]];
      const R rr = alch_sqrt(r2);
      if ((c.parts & kAlchEl) && rr > R(0)) {
        const R rinv = R(1) / rr;
        sgel += (double)(c.rfa ? (qi * t.q) * (rinv + c.krf * r2 - c.crf) : (qi * t.q) * rinv);
      }
      if ((c.parts & kAlchLj) && ab.x != R(0)) {
        R sw, dsw;
        alch_switch(c, rr, sw, dsw);
        const R a6 = c.alpha * (ab.x / ab.y);
#pragma unroll
        for (int q = 0; q < kMaxStates; ++q)
          if (q < S.K) acc[q] += (double)alch_lj_at<R>(r2, ab.x, ab.y, a6, sw, slv[q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kMaxStates; ++q) {
    if (q < S.K) {
      const double s = wave_sum(acc[q]);
      if (lane == 0) so[q] = s;
    }
  }
  const double g = wave_sum(sgel);
  if (lane == 0) so[kMaxStates] = g;
}

// one wave per (replica of the launch, state): sout[r][k] = sum of the blocks' LJ sums at k + lambda_elec,k times their sum of qq g
__global__ __launch_bounds__(64) void alch_states_fold_kernel(const double *__restrict__ spart, int nbA, StateArgs S, int rep0,
                                                              double *__restrict__ sout) {
#pragma clang fp contract(off)
  const int r = rep0 + blockIdx.x, k = blockIdx.y;
  const double *rows = spart + (kMaxStates + 1) * (size_t)r * nbA;
  double g[1] = {0.0}, a[1] = {0.0};
  fold_into<kMaxStates + 1, Sum, Sum>(g, rows + kMaxStates, a, rows + k, nbA);
  g[0] = wave_sum(g[0]), a[0] = wave_sum(a[0]);
  if (threadIdx.x == 0) sout[(size_t)r * kMaxStates + k] = a[0] + S.lam_e[k] * g[0];
}

template <typename R>
AlchConsts<R> consts_of(const tmdhip_ctx *ctx, const AlchState *S) {
  const double zero[3] = {0, 0, 0};
  const PairConsts<R> p = make_consts<R>(ctx, zero);
  AlchConsts<R> c;
  c.r2max = p.r2max;
  c.switch_dist = p.switch_dist, c.inv_switch_range = p.inv_switch_range;
  c.krf = p.krf, c.crf = p.crf;
  c.alpha = (R)S->alpha;
  c.switch_on = p.switch_on, c.switch_reference_mode = p.switch_reference_mode, c.rfa = p.rfa;
  c.parts = ((p.terms & TMDHIP_TERM_LJ) ? kAlchLj : 0u) | ((p.terms & TMDHIP_TERM_ELECTROSTATICS) ? kAlchEl : 0u);
  return c;
}

template <typename R>
Tables<R> tables_of(const tmdhip_ctx *ctx, const AlchState *S) {
  return {S->natoms, S->ns, ctx->d.ntypes, S->slot.as<int32_t>(), ctx->types.as<int32_t>(), ctx->qs.as<R>(),
          ctx->tab.as<typename Vec<R>::T2>(), S->atoms.as<int32_t>(), S->sq.as<R>(), S->scls.as<int32_t>()};
}

// the chunk's boxes (1 / box rounded in the context's precision, as make_consts does), couplings and positions
template <typename R>
ChunkArgs chunk_of(const AlchState *S, int rep_first, int nr, const void *pos, const void *const *pos_each, int c0, const double *box_host) {
  ChunkArgs P;
  const size_t stride = (size_t)S->natoms * 3;
  for (int r = 0; r < kSideChunk; ++r) {
    const bool live = r < nr;
    const double *b = box_host + 3 * (c0 + r);
    const bool allzero = !live || (b[0] == 0 && b[1] == 0 && b[2] == 0);
    for (int k = 0; k < 3; ++k) {
      const R bk = live ? (R)b[k] : R(0);
      P.box[r][k] = (double)bk;
      P.invbox[r][k] = (bk != R(0) && !allzero) ? (double)(R(1) / bk) : 0.0;
    }
    P.lam_v[r] = live ? S->lam_v[rep_first + r] : 1.0;
    P.lam_e[r] = live ? S->lam_e[rep_first + r] : 1.0;
    P.pos[r] = live ? side_pos(pos, pos_each, c0 + r, stride * sizeof(R)) : nullptr;
  }
  return P;
}

// replicas rep0 .. rep0 + nrep - 1; forces / vel point at the rows of replica rep0, box_host at its box; the positions are
// [nrep][N][3] at `pos`, or, with `pos_each`, one array per replica; `out` (double [R][5], indexed by the replica's number)
// wants the energies
template <typename R>
int launch(tmdhip_ctx *ctx, AlchState *S, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host,
           void *forces, void *vel, const void *mass, double kick, double *out, hipStream_t st) {
  const AlchConsts<R> c = consts_of<R>(ctx, S);
  const Tables<R> T = tables_of<R>(ctx, S);
  const size_t stride = (size_t)S->natoms * 3;
  const bool sphere = S->sphere && std::isfinite((double)c.r2max);
  const double *sph = sphere ? S->sph.as<double>() : nullptr;
  const dim3 block(kTile);
  for (int c0 = 0; c0 < nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, nrep - c0), r0 = rep0 + c0;
    const ChunkArgs P = chunk_of<R>(S, r0, nr, pos, pos_each, c0, box_host);
    R *f = forces ? (R *)forces + c0 * stride : nullptr, *v = vel ? (R *)vel + c0 * stride : nullptr;
    if (sphere) hipLaunchKernelGGL(alch_bounds_kernel<R>, dim3((unsigned)nr), block, 0, st, T, P, r0, S->sph.as<double>());
    if (f || v || out)
      hipLaunchKernelGGL(alch_env_kernel<R>, dim3((unsigned)S->nbA, (unsigned)nr), block, 0, st, T, c, P, r0, sph, f, v, (const R *)mass, kick,
                         out ? S->epartA.as<double>() : nullptr);
    if (f || v)
      hipLaunchKernelGGL(alch_solute_kernel<R>, dim3((unsigned)S->nbS, (unsigned)S->nsplit, (unsigned)nr), block, 0, st, T, c, P, r0,
                         S->jchunk, sph, S->part.as<double>());
    // (energies alone: the close kernel adds partials nobody reads, so they may be stale)
    hipLaunchKernelGGL(alch_close_kernel<R>, dim3((unsigned)S->ns, (unsigned)nr), block, 0, st, T, c, P, r0, S->nsplit, S->part.as<double>(),
                       S->off.as<int32_t>(), S->ent.as<AlchEntry>(), f, v, (const R *)mass, kick, out ? S->epartC.as<double>() : nullptr);
    if (out)
      hipLaunchKernelGGL(alch_fold_kernel, dim3((unsigned)nr), dim3(64), 0, st, S->epartA.as<double>(), S->nbA, S->epartC.as<double>(), S->ns,
                         P, r0, out);
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

static_assert(kSideWidth[kSideAlchemy] == 5, "alch_fold_kernel writes five doubles per replica");
AlchState *state_of(tmdhip_ctx *ctx) { return (AlchState *)ctx->side[kSideAlchemy].state; }

int state_check(tmdhip_ctx *ctx) {
  const AlchState *S = state_of(ctx);
  // (what tmdhip_set_alchemical refused may have been switched on since)
  if (S->natoms != ctx->d.natoms || S->nrep != (int)ctx->rep.size() || ctx->nactive < ctx->d.natoms || ctx->vsites || ctx->pme ||
      ctx->side[kSideGb].state)
    return fail("alchemical: the context has changed since tmdhip_set_alchemical (atoms, passive atoms, virtual sites, PME or GB)");
  return 0;
}

int launch_any(tmdhip_ctx *ctx, int rep0, int nrep, const void *pos, const void *const *pos_each, const double *box_host, void *forces,
               void *vel, const void *mass, double kick, double *out, hipStream_t st) {
  AlchState *S = state_of(ctx);
  TMD_TRY(state_check(ctx));
  return ctx->d.dtype == TMDHIP_F32 ? launch<float>(ctx, S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st)
                                    : launch<double>(ctx, S, rep0, nrep, pos, pos_each, box_host, forces, vel, mass, kick, out, st);
}

template <typename R>
int launch_states(tmdhip_ctx *ctx, AlchState *S, const void *pos, const double *box_host, const StateArgs &A, hipStream_t st) {
  const AlchConsts<R> c = consts_of<R>(ctx, S);
  const Tables<R> T = tables_of<R>(ctx, S);
  const bool sphere = S->sphere && std::isfinite((double)c.r2max);
  const double *sph = sphere ? S->sph.as<double>() : nullptr;
  for (int c0 = 0; c0 < S->nrep; c0 += kSideChunk) {
    const int nr = std::min(kSideChunk, S->nrep - c0);
    const ChunkArgs P = chunk_of<R>(S, c0, nr, pos, nullptr, c0, box_host);
    if (sphere) hipLaunchKernelGGL(alch_bounds_kernel<R>, dim3((unsigned)nr), dim3(kTile), 0, st, T, P, c0, S->sph.as<double>());
    hipLaunchKernelGGL(alch_states_kernel<R>, dim3((unsigned)S->nbA, (unsigned)nr), dim3(kTile), 0, st, T, c, P, c0, A, sph,
                       S->spart.as<double>());
    hipLaunchKernelGGL(alch_states_fold_kernel, dim3((unsigned)nr, (unsigned)A.K), dim3(64), 0, st, S->spart.as<double>(), S->nbA, A, c0, S->sout.as<double>());
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int upload(DevBuf &b, const T *src, size_t count) {
  TMD_TRY(b.ensure(std::max<size_t>(sizeof(T) * count, 16)));
  if (count) TMD_HIP(hipMemcpy(b.p, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return 0;
}

template <typename T>
int download(std::vector<T> &dst, const DevBuf &b, size_t count) {
  dst.assign(count, T());
  if (count) TMD_HIP(hipMemcpy(dst.data(), b.p, sizeof(T) * count, hipMemcpyDeviceToHost));
  return 0;
}

int run_check(tmdhip_ctx *ctx, const char *, const double *, const void *, hipStream_t) { return state_check(ctx); }

double *run_energy(tmdhip_ctx *ctx) { return state_of(ctx)->energy.as<double>(); }

void release(tmdhip_ctx *ctx) {
  AlchState *S = state_of(ctx);
  if (!S) return;
  S->release();
  delete S;
  ctx->side[kSideAlchemy] = SideTerm{};
}

}  // namespace

extern "C" {

int tmdhip_set_alchemical(tmdhip_ctx *ctx, const tmdhip_alchemical_desc *desc) {
  if (!ctx || !desc) return fail("tmdhip_set_alchemical: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_alchemical_desc)) return fail("tmdhip_set_alchemical: tmdhip_alchemical_desc size mismatch (ABI)");
  if (!desc->enable) {
    TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the tables may still be in flight)
    release(ctx);
    return 0;
  }
  const int n = ctx->d.natoms, nrep = (int)ctx->rep.size(), ns = desc->natoms, T = ctx->d.ntypes;
  if (desc->nreplicas != nrep) return fail("tmdhip_set_alchemical: nreplicas must be the context's");
  if (ctx->nactive < n) return fail("tmdhip_set_alchemical: not for a context with passive atoms (a brick of the domain decomposition)");
  if (ctx->vsites) return fail("tmdhip_set_alchemical: not for a context with virtual sites");
  if (ctx->pme) return fail("tmdhip_set_alchemical: not with PME (the reciprocal sum has no coupling parameter)");
  if (ctx->side[kSideGb].state) return fail("tmdhip_set_alchemical: not with the generalized-Born model");
  if (ctx->d.terms & (TMDHIP_TERM_REPULSION | TMDHIP_TERM_REPULSIONCG))
    return fail("tmdhip_set_alchemical: not with the repulsion / repulsioncg terms");
  const std::string why = alch_validate(n, nrep, ns, desc->atoms_host, desc->lambda_vdw_host, desc->lambda_elec_host, desc->alpha);
  if (!why.empty()) return fail("tmdhip_set_alchemical: " + why);
  if (!desc->charges_host || !desc->classes_host) return fail("tmdhip_set_alchemical: null charges or classes");
  if (desc->n14 < 0 || (desc->n14 > 0 && (!desc->pair14_host || !desc->scee14_host))) return fail("tmdhip_set_alchemical: bad 1-4 table");
  // the solute in ascending order, with its charges and classes
  std::vector<int32_t> order(ns), atoms(ns), cls(ns), slot(n, -1);
  for (int k = 0; k < ns; ++k) order[k] = k;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return desc->atoms_host[a] < desc->atoms_host[b]; });
  std::vector<double> qs(ns);
  const bool f32 = ctx->d.dtype == TMDHIP_F32;
  const double ke = std::sqrt(kElecFactor);
  for (int t = 0; t < ns; ++t) {
    atoms[t] = desc->atoms_host[order[t]];
    cls[t] = desc->classes_host[order[t]];
    if (cls[t] < 0 || cls[t] >= T) return fail("tmdhip_set_alchemical: a class of the solute is outside the context's table");
    const double q = desc->charges_host[order[t]];
    if (!std::isfinite(q)) return fail("tmdhip_set_alchemical: the charges must be finite");
    qs[t] = f32 ? (double)(float)((double)(float)q * ke) : q * ke;  // (upload_params' rounding)
    slot[atoms[t]] = t;
  }
  for (int64_t p = 0; p < desc->n14; ++p)
    if (!(desc->scee14_host[p] > 0.0) || !std::isfinite(desc->scee14_host[p])) return fail("tmdhip_set_alchemical: every scee must be finite and positive");
  const std::vector<int32_t> pair14(desc->pair14_host, desc->pair14_host + 2 * desc->n14);
  const std::vector<double> scee(desc->scee14_host, desc->scee14_host + desc->n14);
  if (AlchState *S = state_of(ctx)) {
    // the couplings alone have moved (Alchemical.set_lambdas): they travel as kernel arguments, so nothing on the device changes,
    // nothing is synchronised and launches already enqueued keep the couplings they were enqueued with
    if (S->natoms == n && S->nrep == nrep && S->alpha == desc->alpha && S->atoms_h == atoms && S->cls_h == cls && S->qs_h == qs &&
        S->pair14_h == pair14 && S->scee_h == scee) {
      S->lam_v.assign(desc->lambda_vdw_host, desc->lambda_vdw_host + nrep);
      S->lam_e.assign(desc->lambda_elec_host, desc->lambda_elec_host + nrep);
      return 0;
    }
  }
  // closure under the topology: the tuples the caller lists, and the context's own exclusions
  std::string open = alch_closed(slot, desc->pair14_host, desc->n14, 2, "1-4 pair");
  if (open.empty()) open = alch_closed(slot, desc->bond_idx_host, desc->bond_idx_host ? desc->nbonds : 0, 2, "bond");
  if (open.empty()) open = alch_closed(slot, desc->angle_idx_host, desc->angle_idx_host ? desc->nangles : 0, 3, "angle");
  if (open.empty()) open = alch_closed(slot, desc->torsion_idx_host, desc->torsion_idx_host ? desc->ntorsions : 0, 4, "torsion");
  if (!open.empty()) return fail("tmdhip_set_alchemical: " + open);
  for (int64_t p = 0; p < desc->n14; ++p)
    if (slot[desc->pair14_host[2 * p]] < 0) return fail("tmdhip_set_alchemical: 1-4 pair " + std::to_string(p) + " is not the solute's");
  TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the old tables may still be in flight)
  std::vector<int32_t> types_h, eoff, eidx;
  TMD_TRY(download(types_h, ctx->types, (size_t)n));
  TMD_TRY(download(eoff, ctx->excl_off, (size_t)n + 1));
  TMD_TRY(download(eidx, ctx->excl_idx, (size_t)eoff[n]));
  for (int a = 0; a < n; ++a)
    for (int e = eoff[a]; e < eoff[a + 1]; ++e)
      if ((slot[a] >= 0) != (slot[eidx[e]] >= 0))
        return fail("tmdhip_set_alchemical: the exclusion of atoms " + std::to_string(a) + " and " + std::to_string(eidx[e]) +
                    " joins the solute to the environment: the solute must be closed under the topology");
  // the context must not count the solute itself: charge 0 and an all-zero class
  std::vector<double> tabA((size_t)T * T), tabB((size_t)T * T), q_ctx(n);
  if (f32) {
    std::vector<float> tab, q;
    TMD_TRY(download(tab, ctx->tab, (size_t)2 * T * T));
    TMD_TRY(download(q, ctx->qs, (size_t)n));
    for (size_t k = 0; k < (size_t)T * T; ++k) tabA[k] = tab[2 * k], tabB[k] = tab[2 * k + 1];
    for (int i = 0; i < n; ++i) q_ctx[i] = q[i];
  } else {
    std::vector<double> tab;
    TMD_TRY(download(tab, ctx->tab, (size_t)2 * T * T));
    TMD_TRY(download(q_ctx, ctx->qs, (size_t)n));
    for (size_t k = 0; k < (size_t)T * T; ++k) tabA[k] = tab[2 * k], tabB[k] = tab[2 * k + 1];
  }
  std::vector<char> env_class(T, 0);
  for (int i = 0; i < n; ++i) {
    if (slot[i] < 0) {
      env_class[types_h[i]] = 1;
      continue;
    }
    bool null_row = q_ctx[i] == 0.0;
    for (int u = 0; u < T && null_row; ++u) null_row = tabA[(size_t)types_h[i] * T + u] == 0.0 && tabB[(size_t)types_h[i] * T + u] == 0.0;
    if (!null_row)
      return fail("tmdhip_set_alchemical: the context counts solute atom " + std::to_string(i) +
                  " itself: create it with charge 0 and an all-zero Lennard-Jones class for the solute");
  }
  for (int t = 0; t < ns; ++t)
    for (int u = 0; u < T; ++u) {
      const double A = tabA[(size_t)u * T + cls[t]], B = tabB[(size_t)u * T + cls[t]];
      if (env_class[u] && A > 0.0 && !(B > 0.0))
        return fail("tmdhip_set_alchemical: a solute-environment pair has A > 0 >= B: sigma^6 = A / B does not exist");
      if (env_class[u] && A < 0.0) return fail("tmdhip_set_alchemical: a solute-environment pair has A < 0");
    }
  std::vector<int32_t> off;
  std::vector<AlchEntry> ent;
  if (f32)
    alch_build_csr(atoms, eoff.data(), eidx.data(), qs.data(), cls.data(), T, tabA.data(), tabB.data(), desc->n14, desc->pair14_host,
                   desc->scee14_host, [](double a, double b) { return (double)((float)a * (float)b); }, off, ent);
  else
    alch_build_csr(atoms, eoff.data(), eidx.data(), qs.data(), cls.data(), T, tabA.data(), tabB.data(), desc->n14, desc->pair14_host,
                   desc->scee14_host, [](double a, double b) { return a * b; }, off, ent);
  for (const AlchEntry &e : ent)
    if (e.kind == 0 && e.A != 0.0 && !(e.B > 0.0)) return fail("tmdhip_set_alchemical: a solute-solute pair has A != 0 and B <= 0");
  AlchState *S = state_of(ctx);
  if (!S) ctx->side[kSideAlchemy] = SideTerm{S = new AlchState, "alchemical decoupling needs", launch_any, run_check, run_energy, release};
  S->nrep = nrep, S->natoms = n, S->ns = ns;
  S->nbA = (n + kTile - 1) / kTile;
  S->nbS = (ns + kTile - 1) / kTile;
  const char *forced = std::getenv("TMDHIP_ALCHEMY_NSPLIT"), *sphere = std::getenv("TMDHIP_ALCHEMY_SPHERE");
  S->sphere = sphere && std::atoi(sphere) != 0;
  const int want = forced && std::atoi(forced) > 0 ? std::atoi(forced) : kWantWaves / std::max(S->nbS * std::min(nrep, kSideChunk), 1);
  const int ns0 = std::max(1, std::min(want, S->nbA));
  S->jchunk = ((n + ns0 - 1) / ns0 + kTile - 1) / kTile * kTile;
  S->nsplit = (n + S->jchunk - 1) / S->jchunk;
  S->alpha = desc->alpha;
  S->atoms_h = atoms, S->cls_h = cls, S->qs_h = qs, S->pair14_h = pair14, S->scee_h = scee;
  S->lam_v.assign(desc->lambda_vdw_host, desc->lambda_vdw_host + nrep);
  S->lam_e.assign(desc->lambda_elec_host, desc->lambda_elec_host + nrep);
  int rc = upload(S->slot, slot.data(), slot.size());
  if (rc == 0) rc = upload(S->atoms, atoms.data(), atoms.size());
  if (rc == 0) rc = upload(S->scls, cls.data(), cls.size());
  if (rc == 0 && f32) {
    const std::vector<float> q32(qs.begin(), qs.end());
    rc = upload(S->sq, q32.data(), q32.size());
  } else if (rc == 0) {
    rc = upload(S->sq, qs.data(), qs.size());
  }
  if (rc == 0) rc = upload(S->off, off.data(), off.size());
  if (rc == 0) rc = upload(S->ent, ent.data(), ent.size());
  if (rc == 0) rc = S->part.ensure(sizeof(double) * 3 * (size_t)nrep * S->nsplit * ns);
  if (rc == 0) rc = S->epartA.ensure(sizeof(double) * 3 * (size_t)nrep * S->nbA);
  if (rc == 0) rc = S->epartC.ensure(sizeof(double) * (size_t)nrep * ns);
  if (rc == 0) rc = S->sph.ensure(sizeof(double) * 4 * (size_t)nrep);
  if (rc == 0) rc = S->spart.ensure(sizeof(double) * (kMaxStates + 1) * (size_t)nrep * S->nbA);
  if (rc == 0) rc = S->sout.ensure(sizeof(double) * kMaxStates * (size_t)nrep);
  if (rc == 0) rc = S->energy.ensure(sizeof(double) * kSideWidth[kSideAlchemy] * (size_t)nrep);
  if (rc == 0 && hipMemset(S->energy.p, 0, S->energy.bytes) != hipSuccess) rc = fail("tmdhip_set_alchemical: hipMemset failed");
  if (rc == 0 && hipMemset(S->part.p, 0, S->part.bytes) != hipSuccess) rc = fail("tmdhip_set_alchemical: hipMemset failed");
  if (rc != 0) {
    release(ctx);
    return rc;
  }
  TMD_HIP(hipDeviceSynchronize());
  return 0;
}

int tmdhip_alchemical_apply(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, void *forces_dev, void *vel_dev,
                            const void *mass_dev, double kick, double *energies_dev, void *stream) {
  return side_apply(ctx, kSideAlchemy, "tmdhip_alchemical_apply", pos_dev, box_host, forces_dev, vel_dev, mass_dev, kick, energies_dev,
                    stream);
}

int tmdhip_alchemical_energy(tmdhip_ctx *ctx, double *out_host, void *stream) {
  return side_energy(ctx, kSideAlchemy, "tmdhip_alchemical_energy", out_host, stream);
}

int tmdhip_alchemical_states(tmdhip_ctx *ctx, const void *pos_dev, const double *box_host, int32_t nstates, const double *states_host,
                             double *out_host, void *stream) {
  if (!ctx || !pos_dev || !box_host || !states_host || !out_host) return fail("tmdhip_alchemical_states: null argument");
  AlchState *S = state_of(ctx);
  if (!S) return fail("tmdhip_alchemical_states: the context has no alchemical state (tmdhip_set_alchemical)");
  if (nstates < 1 || nstates > kMaxStates) return fail("tmdhip_alchemical_states: between 1 and 32 states per call");
  StateArgs A;
  A.K = nstates;
  for (int k = 0; k < kMaxStates; ++k) {
    A.lam_v[k] = k < nstates ? states_host[2 * k] : 0.0;
    A.lam_e[k] = k < nstates ? states_host[2 * k + 1] : 0.0;
    if (!(A.lam_v[k] >= 0.0 && A.lam_v[k] <= 1.0) || !(A.lam_e[k] >= 0.0 && A.lam_e[k] <= 1.0))
      return fail("tmdhip_alchemical_states: every lambda must lie in [0, 1]");
    if (A.lam_e[k] != 0.0 && A.lam_v[k] != 1.0) return fail("tmdhip_alchemical_states: lambda_elec must be 0 or lambda_vdw must be 1");
  }
  TMD_TRY(state_check(ctx));
  hipStream_t st = (hipStream_t)stream;
  TMD_TRY(ctx->d.dtype == TMDHIP_F32 ? launch_states<float>(ctx, S, pos_dev, box_host, A, st)
                                     : launch_states<double>(ctx, S, pos_dev, box_host, A, st));
  std::vector<double> all((size_t)S->nrep * kMaxStates);
  TMD_HIP(hipMemcpyAsync(all.data(), S->sout.p, sizeof(double) * all.size(), hipMemcpyDeviceToHost, st));
  TMD_HIP(hipStreamSynchronize(st));
  for (int r = 0; r < S->nrep; ++r)
    for (int k = 0; k < nstates; ++k) out_host[(size_t)r * nstates + k] = all[(size_t)r * kMaxStates + k];
  return 0;
}

}  // extern "C"
