// Smooth particle-mesh Ewald (Essmann et al., J. Chem. Phys. 103, 8577 (1995)) for gfx950: the reciprocal-space part of
// the electrostatics term, the excluded-pair correction and the self / background constants.  The real-space part
// erfc(beta r)/r is a branch of pair_terms (pair_math.h) in the generic list and all-pairs kernels.
//
// Per evaluation and replica (pme_apply), all on the caller's stream, behind the pair launch:
//   pme_key_kernel      atom -> bin = its base grid point (floor of the scaled fractional coordinate per axis)
//   radix sort          (bin, atom) pairs, stable: inside a bin the atoms keep ascending index order
//   pme_start_kernel    CSR offsets of the bins (every bin written by exactly one thread, no atomics)
//   pme_theta_kernel    B-spline weights of the atoms in bin order
//   pme_spread_kernel   one thread per grid point GATHERS q theta_x theta_y theta_z of the atoms whose support covers it:
//                       the p^2 z-runs of bins below it, in bin order -> the same floating-point sum on every call
//   R2C FFT, pme_conv_kernel (influence function, energy partial sums per block), C2R FFT
//   pme_force_kernel    one thread per atom: -q grad of its p^3 grid values, added to its own force row
//   pme_excl_kernel     one thread per atom: the excluded-pair correction from its CSR row (both directions stored: the
//                       force on the row's atom; the energy of pairs j > i), added to its own force row
//   pme_energy_kernel   one block: the partial sums in fixed order + self + background -> energies[ELECTROSTATICS]
// Nothing here uses a floating-point atomic: two evaluations of the same input give bit-identical forces and energies.
//
// Conventions (tests/_ewald.py mirrors them): charges are the context's scaled charges q sqrt(k_e); atom i with scaled
// fractional coordinate u = K (s - floor(s)), s = x / L, base floor(u) and w = u - floor(u) contributes M_p(w + j) to grid
// point floor(u) - j (j = 0 .. p-1, periodic); S(m) = sum_k Q(k) exp(-2 pi i m.k / K); E_rec = 1/2 sum_m G(m) |S(m)|^2 with
// G(m) = B(m) exp(-pi^2 |m~|^2 / beta^2) / (pi V |m~|^2), m~ = (m_x / L_x, ...) with signed frequencies, G(0) = 0, and B(m)
// the product of the per-axis moduli 1 / |sum_{k=0}^{p-2} M_p(k+1) exp(2 pi i m k / K)|^2 (a modulus below 1e-7 — odd
// orders at m = K/2 — is replaced by the mean of its neighbours, as OpenMM does).
#include <hipcub/hipcub.hpp>
#include <hipfft/hipfft.h>

#include "engine.h"
#include "virial_math.h"

namespace tmd {

namespace {

constexpr int kPmeThreads = 256;
constexpr int kPmeMaxOrder = 6;

struct PmeRep {
  DevBuf key, val, skey, sval, start, theta, grid, cgrid, infl, epart;
  DevBuf vforce;  // pme_virial: the reciprocal-space force alone, real [N][3] (allocated on first use)
  double infl_box[3] = {-1, -1, -1};
  int64_t evals = 0;
  void release() {
    for (DevBuf *b : {&key, &val, &skey, &sval, &start, &theta, &grid, &cgrid, &infl, &epart, &vforce}) b->release();
  }
};

struct PmeState {
  double beta = 0;
  int K[3] = {0, 0, 0};
  int order = 0;
  int dtype = TMDHIP_F32;
  int key_bits = 1;
  hipfftHandle fwd = 0, bwd = 0;
  size_t fft_work = 0;
  DevBuf moduli;  // double [Kx + Ky + Kz]: B(m) per axis
  DevBuf sort_tmp;
  size_t sort_bytes = 0;
  double sumq = 0, sumq2 = 0;  // of the scaled charges
  std::vector<PmeRep> rep;
  size_t nbins() const { return (size_t)K[0] * K[1] * K[2]; }
  size_t ncomplex() const { return (size_t)K[0] * K[1] * (K[2] / 2 + 1); }
};

template <typename R>
struct PmeBox {
  R L[3], invL[3];
  int K[3];
};

// B-spline weights of order P at the arguments w, w + 1, ..., w + P - 1 (th) and their derivatives (dth)
template <typename R, int P>
__device__ __forceinline__ void bspline(R w, R (&th)[P], R (&dth)[P]) {
  R a[P];
  a[0] = w;
  a[1] = R(1) - w;
#pragma unroll
  for (int j = 2; j < P; ++j) a[j] = R(0);
#pragma unroll
  for (int n = 3; n <= P; ++n) {
    if (n == P) {
#pragma unroll
      for (int j = 0; j < P; ++j) dth[j] = a[j] - (j > 0 ? a[j - 1] : R(0));
    }
    const R inv = R(1) / R(n - 1);
    R b[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const R x = w + R(j);
      const R hi = j < n - 1 ? a[j] : R(0);
      const R lo = j > 0 ? a[j - 1] : R(0);
      b[j] = (x * hi + (R(n) - x) * lo) * inv;
    }
#pragma unroll
    for (int j = 0; j < P; ++j) a[j] = b[j];
  }
#pragma unroll
  for (int j = 0; j < P; ++j) th[j] = a[j];
}

// (no contraction: fused into fma(x, invL, -floor(x * invL)), s is negative when x * invL rounds up to an integer — x = L
// for L = 30 in fp64 — and the atom lands in bin 0 instead of bin K - 1, one grid spacing from where it is)
template <typename R>
__device__ __forceinline__ void frac_coord(R x, R L, R invL, int K, int &iu, R &w) {
#pragma clang fp contract(off)
  R s = x * invL;
  s -= floor(s);
  const R u = s * R(K);
  int b = (int)floor(u);
  w = u - R(b);
  if (b >= K) b -= K;  // (s rounded up to 1)
  if (b < 0) b = 0;
  iu = b;
}

template <typename R>
__global__ __launch_bounds__(kPmeThreads) void pme_key_kernel(int n, const R *__restrict__ pos, PmeBox<R> bx, int *__restrict__ key,
                                                             int *__restrict__ val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int b[3];
  R w;
#pragma unroll
  for (int d = 0; d < 3; ++d) frac_coord<R>(pos[3 * (size_t)i + d], bx.L[d], bx.invL[d], bx.K[d], b[d], w);
  key[i] = (b[0] * bx.K[1] + b[1]) * bx.K[2] + b[2];
  val[i] = i;
}

// start[b] = first sorted slot of bin b, start[nbins] = n: slot s writes the bins in (key[s-1], key[s]]
__global__ __launch_bounds__(kPmeThreads) void pme_start_kernel(int n, int nbins, const int *__restrict__ skey, int *__restrict__ start) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > n) return;
  const int prev = s == 0 ? -1 : skey[s - 1];
  const int cur = s == n ? nbins : skey[s];
  for (int b = prev + 1; b <= cur; ++b) start[b] = s;
}

// theta[s][d * P + j] (d = axis) and theta[s][3 P] = scaled charge, s = sorted slot
template <typename R, int P>
__global__ __launch_bounds__(kPmeThreads) void pme_theta_kernel(int n, const R *__restrict__ pos, const R *__restrict__ qs, PmeBox<R> bx,
                                                               const int *__restrict__ sval, R *__restrict__ theta) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int i = sval[s];
  R *t = theta + (size_t)s * (3 * P + 1);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    int b;
    R w, th[P], dth[P];
    frac_coord<R>(pos[3 * (size_t)i + d], bx.L[d], bx.invL[d], bx.K[d], b, w);
    bspline<R, P>(w, th, dth);
#pragma unroll
    for (int j = 0; j < P; ++j) t[d * P + j] = th[j];
  }
  t[3 * P] = qs[i];
}

// Q(g) = sum over atoms with base b = g + j (per axis, periodic) of q theta_x[jx] theta_y[jy] theta_z[jz]
template <typename R, int P>
__global__ __launch_bounds__(kPmeThreads) void pme_spread_kernel(PmeBox<R> bx, const int *__restrict__ start, const int *__restrict__ skey,
                                                                const R *__restrict__ theta, R *__restrict__ grid) {
  const int Kx = bx.K[0], Ky = bx.K[1], Kz = bx.K[2];
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= Kx * Ky * Kz) return;
  const int gz = g % Kz, gy = (g / Kz) % Ky, gx = g / (Kz * Ky);
  R acc = R(0);
  for (int jx = 0; jx < P; ++jx) {
    int bxi = gx + jx;
    if (bxi >= Kx) bxi -= Kx;
    for (int jy = 0; jy < P; ++jy) {
      int byi = gy + jy;
      if (byi >= Ky) byi -= Ky;
      const int row = (bxi * Ky + byi) * Kz;
      const int z1 = gz + P;
      // the z bins gz .. gz + P - 1: one run of slots, or two when it wraps
      const int s0 = start[row + gz], s1 = start[row + min(z1, Kz)];
      const int s2 = z1 > Kz ? start[row] : 0, s3 = z1 > Kz ? start[row + z1 - Kz] : 0;
      for (int part = 0; part < 2; ++part) {
        const int a = part ? s2 : s0, e = part ? s3 : s1;
        for (int s = a; s < e; ++s) {
          int jz = skey[s] - row - gz;
          if (jz < 0) jz += Kz;
          const R *t = theta + (size_t)s * (3 * P + 1);
          acc += t[3 * P] * t[jx] * t[P + jy] * t[2 * P + jz];
        }
      }
    }
  }
  grid[g] = acc;
}

// G(m) on the half-complex grid
template <typename R>
__global__ __launch_bounds__(kPmeThreads) void pme_influence_kernel(PmeBox<R> bx, double beta, const double *__restrict__ moduli,
                                                                   R *__restrict__ infl) {
  const int Kx = bx.K[0], Ky = bx.K[1], Kz = bx.K[2], Kh = Kz / 2 + 1;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Kx * Ky * Kh) return;
  const int mz = c % Kh, my = (c / Kh) % Ky, mx = c / (Kh * Ky);
  const double fx = (double)(mx <= Kx / 2 ? mx : mx - Kx) / (double)bx.L[0];
  const double fy = (double)(my <= Ky / 2 ? my : my - Ky) / (double)bx.L[1];
  const double fz = (double)mz / (double)bx.L[2];
  const double m2 = fx * fx + fy * fy + fz * fz;
  const double V = (double)bx.L[0] * (double)bx.L[1] * (double)bx.L[2];
  const double pi = 3.141592653589793;
  double G = 0.0;
  if (m2 > 0.0) G = moduli[mx] * moduli[Kx + my] * moduli[Kx + Ky + mz] * exp(-pi * pi * m2 / (beta * beta)) / (pi * V * m2);
  infl[c] = (R)G;
}

static_assert(kPmeThreads == 4 * kWave, "the blocks' sums (reduce.h) meet four waves");

// mode c of the half-complex grid: S(m) *= G(m) in place; its indices, the weight of the mode (2 where the grid leaves the
// conjugate out), G and |S|^2 before the multiplication
struct PmeMode {
  int mx, my, mz;
  double wz, G, s2;
};
template <typename R, typename C>
__device__ __forceinline__ PmeMode conv_mode(int c, int Ky, int Kz, const R *__restrict__ infl, C *__restrict__ cg) {
  const int Kh = Kz / 2 + 1;
  PmeMode m;
  m.mz = c % Kh, m.my = (c / Kh) % Ky, m.mx = c / (Kh * Ky);
  const R G = infl[c];
  C v = cg[c];
  m.wz = (m.mz == 0 || (Kz % 2 == 0 && m.mz == Kz / 2)) ? 1.0 : 2.0;
  m.G = (double)G;
  m.s2 = (double)v.x * (double)v.x + (double)v.y * (double)v.y;
  v.x *= G;
  v.y *= G;
  cg[c] = v;
  return m;
}

// S(m) *= G(m); epart[block] = sum of weight G |S|^2 over the block's points
template <typename R, typename C>
__global__ __launch_bounds__(kPmeThreads) void pme_conv_kernel(int Kx, int Ky, int Kz, const R *__restrict__ infl, C *__restrict__ cg,
                                                              double *__restrict__ epart) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  double e[1] = {0.0};
  if (c < Kx * Ky * (Kz / 2 + 1)) {
    const PmeMode m = conv_mode<R, C>(c, Ky, Kz, infl, cg);
    e[0] = m.wz * m.G * m.s2;
  }
  block_sums<4, Meet::Sequential>(e, epart + blockIdx.x);
}

// F_i = -q_i sum_k grad Q_i(k) phi(k), added to the atom's own row
template <typename R, int P>
__global__ __launch_bounds__(kPmeThreads) void pme_force_kernel(int n, const R *__restrict__ pos, const R *__restrict__ qs, PmeBox<R> bx,
                                                               const R *__restrict__ phi, R *__restrict__ forces) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const R q = qs[i];
  if (q == R(0)) return;
  int b[3];
  R th[3][P], dth[3][P];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    R w;
    frac_coord<R>(pos[3 * (size_t)i + d], bx.L[d], bx.invL[d], bx.K[d], b[d], w);
    bspline<R, P>(w, th[d], dth[d]);
  }
  const int Kx = bx.K[0], Ky = bx.K[1], Kz = bx.K[2];
  R gx = 0, gy = 0, gz = 0;
  for (int jx = 0; jx < P; ++jx) {
    int x = b[0] - jx;
    if (x < 0) x += Kx;
    for (int jy = 0; jy < P; ++jy) {
      int y = b[1] - jy;
      if (y < 0) y += Ky;
      const R *rowp = phi + ((size_t)x * Ky + y) * Kz;
      R s0 = 0, s1 = 0;  // sum_z theta_z phi, sum_z theta_z' phi
#pragma unroll
      for (int jz = 0; jz < P; ++jz) {
        int z = b[2] - jz;
        if (z < 0) z += Kz;
        const R v = rowp[z];
        s0 += th[2][jz] * v;
        s1 += dth[2][jz] * v;
      }
      gx += dth[0][jx] * th[1][jy] * s0;
      gy += th[0][jx] * dth[1][jy] * s0;
      gz += th[0][jx] * th[1][jy] * s1;
    }
  }
  forces[3 * (size_t)i + 0] -= q * gx * (R)Kx * bx.invL[0];
  forces[3 * (size_t)i + 1] -= q * gy * (R)Ky * bx.invL[1];
  forces[3 * (size_t)i + 2] -= q * gz * (R)Kz * bx.invL[2];
}

// erf(x)/x and (2x/sqrt(pi) e^{-x^2} - erf(x)) / x^3, stable for small x
template <typename R>
__device__ __forceinline__ void erf_over_x(R x, R &f0, R &f1) {
  const R tsp = R(1.1283791670955126);  // 2/sqrt(pi)
  if (x < R(2e-2)) {
    const R x2 = x * x;
    f0 = tsp * (R(1) - x2 * (R(1) / R(3) - x2 * (R(0.1) - x2 / R(42))));
    f1 = tsp * (R(-2) / R(3) + x2 * (R(0.4) - x2 * (R(1) / R(7) - x2 / R(27))));
  } else {
    const R e = erf(x), ix = R(1) / x;
    f0 = e * ix;
    f1 = (tsp * x * exp(-x * x) - e) * ix * ix * ix;
  }
}

// excluded pairs: E = -qq erf(beta r)/r once per pair; force on the row's atom from each of its partners
template <typename R>
__global__ __launch_bounds__(kPmeThreads) void pme_excl_kernel(int n, const R *__restrict__ pos, const R *__restrict__ qs,
                                                              const int *__restrict__ excl_off, const int *__restrict__ excl_idx,
                                                              PmeBox<R> bx, R beta, R *__restrict__ forces, double *__restrict__ epart) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double e[1] = {0.0};
  if (i < n) {
    const R qi = qs[i];
    const R xi = pos[3 * (size_t)i], yi = pos[3 * (size_t)i + 1], zi = pos[3 * (size_t)i + 2];
    R fx = 0, fy = 0, fz = 0;
    const int k1 = excl_off[i + 1];
    for (int k = excl_off[i]; k < k1; ++k) {
      const int j = excl_idx[k];
      const R qq = qi * qs[j];
      if (qq == R(0)) continue;
      const R dx = min_image(xi - pos[3 * (size_t)j], bx.L[0], bx.invL[0]);
      const R dy = min_image(yi - pos[3 * (size_t)j + 1], bx.L[1], bx.invL[1]);
      const R dz = min_image(zi - pos[3 * (size_t)j + 2], bx.L[2], bx.invL[2]);
      const R r = sqrt(dx * dx + dy * dy + dz * dz);
      R f0, f1;
      erf_over_x<R>(beta * r, f0, f1);
      // E = -qq beta f0(beta r); dE/dr / r = -qq beta^3 f1(beta r); F_i = -dE/dr d/r
      const R s = qq * beta * beta * beta * f1;
      fx += s * dx;
      fy += s * dy;
      fz += s * dz;
      if (j > i) e[0] -= (double)(qq * beta * f0);
    }
    if (forces) {
      forces[3 * (size_t)i + 0] += fx;
      forces[3 * (size_t)i + 1] += fy;
      forces[3 * (size_t)i + 2] += fz;
    }
  }
  block_sums<4, Meet::Sequential>(e, epart + blockIdx.x);
}

// energies[ELECTROSTATICS] += 1/2 sum(conv partials) + sum(exclusion partials) + constant, in a fixed order (the partials taken
// 256 apart by the block's threads, not by reduce.h's fold)
__global__ __launch_bounds__(kPmeThreads) void pme_energy_kernel(const double *__restrict__ conv, int nconv, const double *__restrict__ excl,
                                                                int nexcl, double konst, double *__restrict__ energies) {
  double a = 0.0, b = 0.0;
  for (int k = threadIdx.x; k < nconv; k += kPmeThreads) a += conv[k];
  for (int k = threadIdx.x; k < nexcl; k += kPmeThreads) b += excl[k];
  const double s = block_sum<Meet::Sequential>(0.5 * a + b);
  if (threadIdx.x == 0) energies[TMDHIP_E_ELECTROSTATICS] += s + konst;
}

// B-spline moduli of one axis (host, double)
std::vector<double> bspline_moduli(int K, int p) {
  // M_p at the integers 0 .. p-1 by the same recursion as the device (w = 0)
  std::vector<double> a(p, 0.0), b(p);
  a[0] = 0.0;
  a[1] = 1.0;
  for (int n = 3; n <= p; ++n) {
    for (int j = 0; j < p; ++j) {
      const double x = j, hi = j < n - 1 ? a[j] : 0.0, lo = j > 0 ? a[j - 1] : 0.0;
      b[j] = (x * hi + (n - x) * lo) / (n - 1);
    }
    a = b;
  }
  std::vector<double> mod(K);
  const double pi = 3.141592653589793;
  for (int m = 0; m < K; ++m) {
    double re = 0, im = 0;
    for (int k = 0; k <= p - 2; ++k) {
      const double arg = 2 * pi * m * k / K;
      re += a[k + 1] * std::cos(arg);
      im += a[k + 1] * std::sin(arg);
    }
    mod[m] = re * re + im * im;
  }
  for (int m = 0; m < K; ++m)
    if (mod[m] < 1e-7) mod[m] = 0.5 * (mod[(m - 1 + K) % K] + mod[(m + 1) % K]);
  for (int m = 0; m < K; ++m) mod[m] = 1.0 / mod[m];
  return mod;
}

int alloc_rep(PmeState &P, PmeRep &pr, int n) {
  const size_t rs = P.dtype == TMDHIP_F32 ? 4 : 8;
  const size_t nb = P.nbins(), nc = P.ncomplex();
  TMD_TRY(pr.key.ensure(sizeof(int) * n));
  TMD_TRY(pr.val.ensure(sizeof(int) * n));
  TMD_TRY(pr.skey.ensure(sizeof(int) * n));
  TMD_TRY(pr.sval.ensure(sizeof(int) * n));
  TMD_TRY(pr.start.ensure(sizeof(int) * (nb + 1)));
  TMD_TRY(pr.theta.ensure(rs * (3 * P.order + 1) * (size_t)n));
  TMD_TRY(pr.grid.ensure(rs * nb));
  TMD_TRY(pr.cgrid.ensure(2 * rs * nc));
  TMD_TRY(pr.infl.ensure(rs * nc));
  const size_t nconv = (nc + kPmeThreads - 1) / kPmeThreads, nex = ((size_t)n + kPmeThreads - 1) / kPmeThreads;
  TMD_TRY(pr.epart.ensure(sizeof(double) * (nconv + nex)));
  return 0;
}

// key ... forward FFT: S(m) of the replica's charges in pr.cgrid (both FFT plans are put on the stream)
template <typename R, int P>
int pme_forward(tmdhip_ctx *ctx, PmeState &S, PmeRep &pr, const R *pos, const PmeBox<R> &bx, hipStream_t st) {
  const int n = ctx->d.natoms;
  const int nb = (int)S.nbins();
  const unsigned ga = (unsigned)((n + kPmeThreads - 1) / kPmeThreads);
  const R *qs = ctx->qs.as<R>();
  hipLaunchKernelGGL((pme_key_kernel<R>), dim3(ga), dim3(kPmeThreads), 0, st, n, pos, bx, pr.key.as<int>(), pr.val.as<int>());
  TMD_HIP(hipGetLastError());
  size_t tmp = S.sort_bytes;
  TMD_HIP(hipcub::DeviceRadixSort::SortPairs(S.sort_tmp.p, tmp, pr.key.as<int>(), pr.skey.as<int>(), pr.val.as<int>(), pr.sval.as<int>(), n,
                                             0, S.key_bits, st));
  hipLaunchKernelGGL(pme_start_kernel, dim3((unsigned)((n + 1 + kPmeThreads - 1) / kPmeThreads)), dim3(kPmeThreads), 0, st, n, nb,
                     pr.skey.as<int>(), pr.start.as<int>());
  hipLaunchKernelGGL((pme_theta_kernel<R, P>), dim3(ga), dim3(kPmeThreads), 0, st, n, pos, qs, bx, pr.sval.as<int>(), pr.theta.as<R>());
  hipLaunchKernelGGL((pme_spread_kernel<R, P>), dim3((unsigned)((nb + kPmeThreads - 1) / kPmeThreads)), dim3(kPmeThreads), 0, st, bx,
                     pr.start.as<int>(), pr.skey.as<int>(), pr.theta.as<R>(), pr.grid.as<R>());
  TMD_HIP(hipGetLastError());
  if (hipfftSetStream(S.fwd, st) != HIPFFT_SUCCESS || hipfftSetStream(S.bwd, st) != HIPFFT_SUCCESS) return fail("PME: hipfftSetStream failed");
  hipfftResult fr;
  if constexpr (std::is_same<R, float>::value)
    fr = hipfftExecR2C(S.fwd, pr.grid.as<hipfftReal>(), pr.cgrid.as<hipfftComplex>());
  else
    fr = hipfftExecD2Z(S.fwd, pr.grid.as<hipfftDoubleReal>(), pr.cgrid.as<hipfftDoubleComplex>());
  if (fr != HIPFFT_SUCCESS) return fail("PME: forward FFT failed (" + std::to_string((int)fr) + ")");
  return 0;
}

// the inverse FFT: pr.cgrid -> pr.grid
template <typename R>
int pme_inverse(PmeState &S, PmeRep &pr) {
  hipfftResult fr;
  if constexpr (std::is_same<R, float>::value)
    fr = hipfftExecC2R(S.bwd, pr.cgrid.as<hipfftComplex>(), pr.grid.as<hipfftReal>());
  else
    fr = hipfftExecZ2D(S.bwd, pr.cgrid.as<hipfftDoubleComplex>(), pr.grid.as<hipfftDoubleReal>());
  if (fr != HIPFFT_SUCCESS) return fail("PME: inverse FFT failed (" + std::to_string((int)fr) + ")");
  return 0;
}

template <typename R, int P>
int apply_order(tmdhip_ctx *ctx, PmeState &S, PmeRep &pr, const R *pos, const PmeBox<R> &bx, R *forces, double *energies,
                hipStream_t st) {
  const int n = ctx->d.natoms;
  const int nc = (int)S.ncomplex();
  const unsigned ga = (unsigned)((n + kPmeThreads - 1) / kPmeThreads);
  const R *qs = ctx->qs.as<R>();
  TMD_TRY((pme_forward<R, P>(ctx, S, pr, pos, bx, st)));
  double *epart = pr.epart.as<double>();
  const int nconv = (nc + kPmeThreads - 1) / kPmeThreads, nex = (int)ga;
  using C = typename std::conditional<std::is_same<R, float>::value, hipfftComplex, hipfftDoubleComplex>::type;
  hipLaunchKernelGGL((pme_conv_kernel<R, C>), dim3((unsigned)nconv), dim3(kPmeThreads), 0, st, S.K[0], S.K[1], S.K[2], pr.infl.as<R>(),
                     pr.cgrid.as<C>(), epart);
  TMD_HIP(hipGetLastError());
  if (forces) {
    TMD_TRY(pme_inverse<R>(S, pr));
    hipLaunchKernelGGL((pme_force_kernel<R, P>), dim3(ga), dim3(kPmeThreads), 0, st, n, pos, qs, bx, pr.grid.as<R>(), forces);
    TMD_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL((pme_excl_kernel<R>), dim3(ga), dim3(kPmeThreads), 0, st, n, pos, qs, ctx->excl_off.as<int>(), ctx->excl_idx.as<int>(),
                     bx, (R)S.beta, forces, epart + nconv);
  TMD_HIP(hipGetLastError());
  if (energies) {
    const double V = (double)bx.L[0] * (double)bx.L[1] * (double)bx.L[2], pi = 3.141592653589793;
    const double konst = -S.beta / std::sqrt(pi) * S.sumq2 - pi * S.sumq * S.sumq / (2.0 * V * S.beta * S.beta);
    hipLaunchKernelGGL(pme_energy_kernel, dim3(1), dim3(kPmeThreads), 0, st, epart, nconv, epart + nconv, nex, konst, energies);
    TMD_HIP(hipGetLastError());
  }
  return 0;
}

// ---- the reciprocal-space part of the molecular virial (virial.hip: tmdhip_pressure) -------------------------------------
// pme_conv_kernel's modes (conv_mode) with three per-block partials of e(m) [1 - 2 (1 + pi^2 m^2 / beta^2) m_a^2 / m^2], e(m) = w_z G |S|^2 / 2
template <typename R, typename C>
__global__ __launch_bounds__(kPmeThreads) void pme_conv_virial_kernel(PmeBox<R> bx, double beta, const R *__restrict__ infl, C *__restrict__ cg,
                                                                     double *__restrict__ vpart) {
  const int Kx = bx.K[0], Ky = bx.K[1], Kz = bx.K[2];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  double w[3] = {0.0, 0.0, 0.0};
  if (c < Kx * Ky * (Kz / 2 + 1)) {
    const PmeMode m = conv_mode<R, C>(c, Ky, Kz, infl, cg);
    const double e = 0.5 * m.wz * m.G * m.s2;
    const double f[3] = {(double)(m.mx <= Kx / 2 ? m.mx : m.mx - Kx) / (double)bx.L[0],
                         (double)(m.my <= Ky / 2 ? m.my : m.my - Ky) / (double)bx.L[1], (double)m.mz / (double)bx.L[2]};
    const double m2 = f[0] * f[0] + f[1] * f[1] + f[2] * f[2];
    if (m2 > 0.0)
      for (int a = 0; a < 3; ++a) w[a] = e * virial_mode_factor(m2, f[a] * f[a], beta);
  }
  block_sums<4, Meet::Sequential>(w, vpart + 3 * (size_t)blockIdx.x);
}

// one thread per atom: -delta_i,a F^rec_i,a, per-block partials; block 0 also stores the background's share (E ~ 1 / V: its
// own value on every diagonal element) in the slot behind the last block
template <typename R>
__global__ __launch_bounds__(kPmeThreads) void pme_virial_atoms_kernel(int n, const R *__restrict__ pos, const R *__restrict__ frec,
                                                                      const int *__restrict__ mol_of, const double *__restrict__ centre,
                                                                      double background, double *__restrict__ vpart) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double w[3] = {0.0, 0.0, 0.0};
  if (i < n) {
    const double *c = centre + 3 * (size_t)mol_of[i];
    for (int a = 0; a < 3; ++a) w[a] = -(((double)pos[3 * (size_t)i + a] - c[a]) * (double)frec[3 * (size_t)i + a]);
  }
  block_sums<4, Meet::Sequential>(w, vpart + 3 * (size_t)blockIdx.x);
  if (blockIdx.x == 0 && threadIdx.x < 3) vpart[3 * (size_t)gridDim.x + threadIdx.x] = background;
}

template <typename R, int P>
int virial_order(tmdhip_ctx *ctx, PmeState &S, PmeRep &pr, const R *pos, const PmeBox<R> &bx, const int *mol_of, const double *centre,
                 double *vpart, hipStream_t st) {
  const int n = ctx->d.natoms;
  const int nc = (int)S.ncomplex();
  const unsigned ga = (unsigned)((n + kPmeThreads - 1) / kPmeThreads);
  const R *qs = ctx->qs.as<R>();
  TMD_TRY(pr.vforce.ensure(sizeof(R) * 3 * (size_t)n));
  TMD_TRY((pme_forward<R, P>(ctx, S, pr, pos, bx, st)));
  const int nconv = (nc + kPmeThreads - 1) / kPmeThreads;
  using C = typename std::conditional<std::is_same<R, float>::value, hipfftComplex, hipfftDoubleComplex>::type;
  hipLaunchKernelGGL((pme_conv_virial_kernel<R, C>), dim3((unsigned)nconv), dim3(kPmeThreads), 0, st, bx, S.beta, pr.infl.as<R>(),
                     pr.cgrid.as<C>(), vpart);
  TMD_HIP(hipGetLastError());
  TMD_TRY(pme_inverse<R>(S, pr));
  TMD_HIP(hipMemsetAsync(pr.vforce.p, 0, sizeof(R) * 3 * (size_t)n, st));
  hipLaunchKernelGGL((pme_force_kernel<R, P>), dim3(ga), dim3(kPmeThreads), 0, st, n, pos, qs, bx, pr.grid.as<R>(), pr.vforce.as<R>());
  const double V = (double)bx.L[0] * (double)bx.L[1] * (double)bx.L[2], pi = 3.141592653589793;
  const double background = -pi * S.sumq * S.sumq / (2.0 * V * S.beta * S.beta);
  hipLaunchKernelGGL((pme_virial_atoms_kernel<R>), dim3(ga), dim3(kPmeThreads), 0, st, n, pos, pr.vforce.as<R>(), mol_of, centre, background,
                     vpart + 3 * (size_t)nconv);
  TMD_HIP(hipGetLastError());
  return 0;
}

// the box as the kernels take it; brings the replica's influence function up to date with it
template <typename R>
int pme_box_for(PmeState &S, PmeRep &pr, const double *box, hipStream_t st, PmeBox<R> &bx) {
  for (int d = 0; d < 3; ++d) {
    bx.L[d] = (R)box[d];
    bx.invL[d] = R(1) / bx.L[d];
    bx.K[d] = S.K[d];
  }
  if (box[0] != pr.infl_box[0] || box[1] != pr.infl_box[1] || box[2] != pr.infl_box[2]) {  // C(m) of this box
    const int nc = (int)S.ncomplex();
    hipLaunchKernelGGL((pme_influence_kernel<R>), dim3((unsigned)((nc + kPmeThreads - 1) / kPmeThreads)), dim3(kPmeThreads), 0, st, bx, S.beta,
                       S.moduli.as<double>(), pr.infl.as<R>());
    TMD_HIP(hipGetLastError());
    for (int d = 0; d < 3; ++d) pr.infl_box[d] = box[d];
  }
  return 0;
}

}  // namespace

// entries [3] of the partials pme_virial writes per replica (0 without PME)
int pme_virial_partials(const tmdhip_ctx *ctx) {
  if (!ctx->pme) return 0;
  const PmeState &S = *static_cast<const PmeState *>(ctx->pme);
  return (int)((S.ncomplex() + kPmeThreads - 1) / kPmeThreads) + (ctx->d.natoms + kPmeThreads - 1) / kPmeThreads + 1;
}

// The reciprocal-space part of replica r's molecular virial as pme_virial_partials() x 3 doubles at `vpart`: the modes' W^rec
// (pme_forward, then pme_conv_virial_kernel), -delta_i . F^rec_i from pme_inverse + pme_force_kernel into a zeroed scratch array, and the neutralising background.  The self term has no volume dependence; the
// excluded-pair correction is intramolecular and does not enter.  mol_of / centre: virial.hip's tables (centre: this replica's).
template <typename R>
int pme_virial(tmdhip_ctx *ctx, int r, const R *pos, const double *box, const int *mol_of, const double *centre, double *vpart,
               hipStream_t st) {
  if (!ctx->pme) return 0;
  PmeState &S = *static_cast<PmeState *>(ctx->pme);
  if (!(box[0] > 0 && box[1] > 0 && box[2] > 0)) return fail("PME needs a periodic box (all three edges > 0)");
  if (r < 0 || r >= (int)S.rep.size()) return fail("PME: bad replica index");
  PmeRep &pr = S.rep[r];
  PmeBox<R> bx;
  TMD_TRY(pme_box_for<R>(S, pr, box, st, bx));
  switch (S.order) {
    case 4: return virial_order<R, 4>(ctx, S, pr, pos, bx, mol_of, centre, vpart, st);
    case 5: return virial_order<R, 5>(ctx, S, pr, pos, bx, mol_of, centre, vpart, st);
    default: return virial_order<R, 6>(ctx, S, pr, pos, bx, mol_of, centre, vpart, st);
  }
}

template int pme_virial<float>(tmdhip_ctx *, int, const float *, const double *, const int *, const double *, double *, hipStream_t);
template int pme_virial<double>(tmdhip_ctx *, int, const double *, const double *, const int *, const double *, double *, hipStream_t);

template <typename R>
int pme_apply(tmdhip_ctx *ctx, int r, const R *pos, const double *box, R *forces, double *energies, hipStream_t st) {
  if (!ctx->pme || (!forces && !energies)) return 0;
  PmeState &S = *static_cast<PmeState *>(ctx->pme);
  if (!(box[0] > 0 && box[1] > 0 && box[2] > 0)) return fail("PME needs a periodic box (all three edges > 0)");
  if (r < 0 || r >= (int)S.rep.size()) return fail("PME: bad replica index");
  PmeRep &pr = S.rep[r];
  PmeBox<R> bx;
  TMD_TRY(pme_box_for<R>(S, pr, box, st, bx));
  pr.evals++;
  switch (S.order) {
    case 4: return apply_order<R, 4>(ctx, S, pr, pos, bx, forces, energies, st);
    case 5: return apply_order<R, 5>(ctx, S, pr, pos, bx, forces, energies, st);
    default: return apply_order<R, 6>(ctx, S, pr, pos, bx, forces, energies, st);
  }
}

template int pme_apply<float>(tmdhip_ctx *, int, const float *, const double *, float *, double *, hipStream_t);
template int pme_apply<double>(tmdhip_ctx *, int, const double *, const double *, double *, double *, hipStream_t);

int pme_hook(tmdhip_ctx *ctx, int r, const void *pos, const double *box, void *forces, double *energies, int flags, hipStream_t st) {
  if (!ctx->pme) return 0;
  void *f = (flags & TMDHIP_WANT_FORCES) ? forces : nullptr;
  double *e = (flags & TMDHIP_WANT_ENERGY) ? energies : nullptr;
  return ctx->d.dtype == TMDHIP_F32 ? pme_apply<float>(ctx, r, (const float *)pos, box, (float *)f, e, st)
                                    : pme_apply<double>(ctx, r, (const double *)pos, box, (double *)f, e, st);
}

void pme_release(tmdhip_ctx *ctx) {
  if (!ctx || !ctx->pme) return;
  PmeState *S = static_cast<PmeState *>(ctx->pme);
  (void)hipDeviceSynchronize();
  if (S->fwd) (void)hipfftDestroy(S->fwd);
  if (S->bwd) (void)hipfftDestroy(S->bwd);
  for (auto &pr : S->rep) pr.release();
  S->moduli.release();
  S->sort_tmp.release();
  delete S;
  ctx->pme = nullptr;
  ctx->pme_beta = 0;
}

int64_t pme_evaluations(const tmdhip_ctx *ctx, int r) {
  if (!ctx->pme) return 0;
  const PmeState &S = *static_cast<const PmeState *>(ctx->pme);
  return r >= 0 && r < (int)S.rep.size() ? S.rep[r].evals : 0;
}

int64_t pme_bytes(const tmdhip_ctx *ctx) {
  if (!ctx->pme) return 0;
  const PmeState &S = *static_cast<const PmeState *>(ctx->pme);
  int64_t b = (int64_t)(S.moduli.bytes + S.sort_tmp.bytes + S.fft_work);
  for (const auto &pr : S.rep)
    for (const DevBuf *d : {&pr.key, &pr.val, &pr.skey, &pr.sval, &pr.start, &pr.theta, &pr.grid, &pr.cgrid, &pr.infl, &pr.epart, &pr.vforce})
      b += (int64_t)d->bytes;
  return b;
}

}  // namespace tmd

extern "C" int tmdhip_set_pme(tmdhip_ctx *ctx, const tmdhip_pme_desc *desc) {
  using namespace tmd;
  if (!ctx || !desc) return fail("tmdhip_set_pme: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_pme_desc)) return fail("tmdhip_set_pme: tmdhip_pme_desc size mismatch (ABI)");
  pme_release(ctx);
  if (!desc->enable) return 0;
  if (!(ctx->d.cutoff > 0)) return fail("tmdhip_set_pme: PME needs a cutoff");
  if (ctx->d.rfa) return fail("tmdhip_set_pme: PME and reaction field exclude each other");
  if (!(ctx->d.terms & TMDHIP_TERM_ELECTROSTATICS)) return fail("tmdhip_set_pme: PME needs the electrostatics term");
  if (desc->order < 4 || desc->order > kPmeMaxOrder) return fail("tmdhip_set_pme: order must be 4 .. 6");
  if (!(desc->beta > 0)) return fail("tmdhip_set_pme: beta must be positive");
  for (int d = 0; d < 3; ++d)
    if (desc->grid[d] < desc->order || desc->grid[d] > 1024) return fail("tmdhip_set_pme: grid edges must lie in [order, 1024]");
  const int n = ctx->d.natoms;
  auto *S = new PmeState();
  S->beta = desc->beta;
  S->order = desc->order;
  S->dtype = ctx->d.dtype;
  for (int d = 0; d < 3; ++d) S->K[d] = desc->grid[d];
  if (S->nbins() >= (size_t)1 << 30) {
    delete S;
    return fail("tmdhip_set_pme: grid too large");
  }
  ctx->pme = S;  // (pme_release cleans up from here on)
  auto bail = [&](int rc) {
    pme_release(ctx);
    return rc;
  };
  while (((size_t)1 << S->key_bits) < S->nbins()) S->key_bits++;
  // charge sums of the self and background terms, from the scaled charges the kernels use
  const bool f32 = ctx->d.dtype == TMDHIP_F32;
  std::vector<double> q(n);
  if (f32) {
    std::vector<float> h(n);
    if (hipMemcpy(h.data(), ctx->qs.p, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess) return bail(fail("tmdhip_set_pme: charge read-back failed"));
    for (int i = 0; i < n; ++i) q[i] = h[i];
  } else if (hipMemcpy(q.data(), ctx->qs.p, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) {
    return bail(fail("tmdhip_set_pme: charge read-back failed"));
  }
  for (int i = 0; i < n; ++i) {
    S->sumq += q[i];
    S->sumq2 += q[i] * q[i];
  }
  std::vector<double> mod;
  for (int d = 0; d < 3; ++d) {
    const std::vector<double> m = bspline_moduli(S->K[d], S->order);
    mod.insert(mod.end(), m.begin(), m.end());
  }
  if (S->moduli.ensure(sizeof(double) * mod.size())) return bail(-1);
  if (hipMemcpy(S->moduli.p, mod.data(), sizeof(double) * mod.size(), hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail("tmdhip_set_pme: moduli upload failed"));
  S->rep.resize(ctx->rep.size());
  for (auto &pr : S->rep)
    if (alloc_rep(*S, pr, n)) return bail(-1);
  size_t tmp = 0;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (int *)nullptr, (int *)nullptr, (int *)nullptr, (int *)nullptr, n, 0, S->key_bits) !=
      hipSuccess)
    return bail(fail("tmdhip_set_pme: radix sort size query failed"));
  S->sort_bytes = std::max<size_t>(tmp, 16);
  if (S->sort_tmp.ensure(S->sort_bytes)) return bail(-1);
  // the FFT plans: rocFFT builds (or loads) its kernels here, outside every timed evaluation
  const hipfftType tf = f32 ? HIPFFT_R2C : HIPFFT_D2Z, tb = f32 ? HIPFFT_C2R : HIPFFT_Z2D;
  if (hipfftPlan3d(&S->fwd, S->K[0], S->K[1], S->K[2], tf) != HIPFFT_SUCCESS ||
      hipfftPlan3d(&S->bwd, S->K[0], S->K[1], S->K[2], tb) != HIPFFT_SUCCESS)
    return bail(fail("tmdhip_set_pme: hipFFT plan creation failed"));
  size_t w0 = 0, w1 = 0;
  (void)hipfftGetSize(S->fwd, &w0);
  (void)hipfftGetSize(S->bwd, &w1);
  S->fft_work = w0 + w1;
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail("tmdhip_set_pme: device synchronisation failed"));
  ctx->pme_beta = desc->beta;
  return 0;
}
