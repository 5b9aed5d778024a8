// Instantaneous pressure: the molecular virial of the nonbonded force field and the kinetic term of the molecules' centres, for
// gfx950 (tmdhip_set_molecules, tmdhip_pressure; the per-pair arithmetic: virial_math.h).
//
//   P_aa V = sum_I M_I V_I,a^2 + W_aa,   W_aa = 1/2 sum_i sum_{j in list(i)} d_ij,a f_ij,a - sum_i delta_i,a F_i,a
// with R_I / V_I the mass-weighted centre of molecule I and its velocity and delta_i = r_i - R_I(i).  Under a rigid displacement of
// whole molecules the bonded terms, the constraint forces and every other intramolecular force do no work, so none of them
// appears; molecules must be whole (no minimum image inside a molecule: the barostat's contract).
//
// Separate launches between two tmdhip_md_run calls, like a plain evaluation; no pair, step or list-build kernel is touched.
//   mol_centre_kernel      one thread per molecule of <= 64 atoms (one wave per larger one: a second launch, only when such
//                          molecules exist), blockIdx.y = replica: R_I in double, per-block partials of sum M_I V_I,a^2
//   virial_list_kernel     the twin of list_pair_kernel<R, false, LPA, 0> (pair_generic.hip): the same row addressing, entry
//                          decoding, unroll, predication and pair_terms; every lane adds f_a (d_a / 2 - delta_i,a) pair by pair
//                          in double; wave butterfly, the four waves meet in LDS, one thread stores the block's three partials
//   virial_allpairs_kernel the twin of allpairs_kernel: all-pairs contexts and cell-list contexts that fell back
//   pme.hip: pme_virial    PME contexts: the modes' W^rec from a twin of the convolution kernel, -delta_i . F^rec_i from the usual
//                          C2R + force kernel into a scratch array, and the neutralising background, as partials of their own
//   virial_fold_kernel     one wave per replica: lane l sums the partials l, l + 64, ..., then the butterfly; writes
//                          double [R][8] = (sum M V^2 x, y, z; W x, y, z; V; P)
// No floating-point atomics anywhere, every sum in one fixed order: two calls on the same state give the same bits.
// The pair kernels are bound like the generic list kernel they copy (gather latency + pair_terms); everything else is a few
// microseconds of launch.
#include "engine.h"
#include "virial_math.h"

using namespace tmd;

namespace {

constexpr int kThreads = 256;
constexpr int kBigMol = 64;

struct VirialState {
  int nmol = 0, natoms = 0, nbig = 0, kblocks = 0;
  DevBuf off, mem, mol_of, big;  // the CSR, atom -> molecule, the molecules of more than kBigMol atoms
  DevBuf centre;                 // double [R][nmol][3]
  DevBuf kpart;                  // double [R][kblocks][3]
  DevBuf wpart;                  // double [R][wstride][3]
  DevBuf xpart;                  // double [R][xstride][3]: the reciprocal-space PME part (pme.hip: pme_virial)
  DevBuf boxes;                  // double [R][3]
  DevBuf out;                    // double [R][8]
  std::vector<int32_t> off_h, mem_h;
  const void *mass_checked = nullptr;  // the mass array whose molecules are known to have mass
  void release() {
    for (DevBuf *b : {&off, &mem, &mol_of, &big, &centre, &kpart, &wpart, &xpart, &boxes, &out}) b->release();
  }
};

// block-wide meeting of three per-lane doubles: dst[0..2] = the block's sums, in one fixed order
template <int WAVES>
__device__ __forceinline__ void block_store3(double a, double b, double c, double *dst) {
#pragma clang fp contract(off)
  __shared__ double part[WAVES][3];
  a = wave_sum(a), b = wave_sum(b), c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = a;
    part[threadIdx.x >> 6][1] = b;
    part[threadIdx.x >> 6][2] = c;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = part[0][threadIdx.x];
    if (WAVES == 4) s = (s + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    dst[threadIdx.x] = s;
  }
}

// big_pass = 0: thread = molecule (those of more than kBigMol atoms are left out), grid.x = ceil(nmol / 256);
// big_pass = 1: block of one wave = big[blockIdx.x].  blockIdx.y = replica.  vel may be null (no kinetic term).
template <typename R>
__global__ __launch_bounds__(kThreads) void mol_centre_kernel(int natoms, int nmol, const int *__restrict__ off,
                                                              const int *__restrict__ mem, const int *__restrict__ big,
                                                              const R *__restrict__ pos, const R *__restrict__ vel,
                                                              const R *__restrict__ mass, double *__restrict__ centre,
                                                              double *__restrict__ kpart, int kblocks, int small_blocks, int big_pass) {
#pragma clang fp contract(off)
  const int r = blockIdx.y;
  const size_t base = (size_t)r * natoms * 3;
  const R *p = pos + base;
  const R *v = vel ? vel + base : nullptr;
  int g, first, stride, e = 0;
  bool work;
  if (!big_pass) {
    g = blockIdx.x * kThreads + threadIdx.x;
    work = g < nmol;
    first = work ? off[g] : 0;
    e = work ? off[g + 1] : 0;
    work = work && e - first <= kBigMol;
    stride = 1;
  } else {
    g = big[blockIdx.x];
    first = off[g] + (int)threadIdx.x, e = off[g + 1], stride = kWave;
    work = true;
  }
  double sm = 0, sx = 0, sy = 0, sz = 0, px = 0, py = 0, pz = 0;
  if (work)
    for (int k = first; k < e; k += stride) {
      const int a = mem[k];
      const double m = (double)mass[a];
      sm += m;
      sx += m * (double)p[3 * a], sy += m * (double)p[3 * a + 1], sz += m * (double)p[3 * a + 2];
      if (v) px += m * (double)v[3 * a], py += m * (double)v[3 * a + 1], pz += m * (double)v[3 * a + 2];
    }
  if (big_pass) {
    sm = wave_sum(sm), sx = wave_sum(sx), sy = wave_sum(sy), sz = wave_sum(sz);
    px = wave_sum(px), py = wave_sum(py), pz = wave_sum(pz);
    work = threadIdx.x == 0;
  }
  double kx = 0, ky = 0, kz = 0;
  if (work) {
    double *c = centre + ((size_t)r * nmol + g) * 3;
    c[0] = sx / sm, c[1] = sy / sm, c[2] = sz / sm;
    // M V_a^2 = (sum m v_a)^2 / M
    kx = px * px / sm, ky = py * py / sm, kz = pz * pz / sm;
  }
  double *dst = kpart + ((size_t)r * kblocks + (big_pass ? small_blocks + blockIdx.x : blockIdx.x)) * 3;
  if (big_pass) {
    if (threadIdx.x == 0) dst[0] = kx, dst[1] = ky, dst[2] = kz;
  } else {
    block_store3<kThreads / 64>(kx, ky, kz, dst);
  }
}

// offset of atom `i` (at x, y, z) from its molecule's centre
template <typename R>
__device__ __forceinline__ void centre_offset(const int *__restrict__ mol_of, const double *__restrict__ centre, int i, R x, R y, R z,
                                              double (&delta)[3]) {
#pragma clang fp contract(off)
  const double *c = centre + 3 * (size_t)mol_of[i];
  delta[0] = (double)x - c[0], delta[1] = (double)y - c[1], delta[2] = (double)z - c[2];
}

// list_pair_kernel<R, false, LPA, 0> with the force accumulation replaced by the virial's; wpart: this replica's [blocks][3]
template <typename R, int LPA>
__global__ __launch_bounds__(256) void virial_list_kernel(int n, const typename Vec<R>::T4 *__restrict__ sorted, const int *__restrict__ stype,
                                                          const int *__restrict__ order, int ntypes,
                                                          const typename Vec<R>::T2 *__restrict__ tab, const unsigned *__restrict__ nlist,
                                                          const int *__restrict__ nneigh, int maxn, PairConsts<R> c,
                                                          const int *__restrict__ mol_of, const double *__restrict__ centre,
                                                          double *__restrict__ wpart) {
  using R4 = typename Vec<R>::T4;
  using R2 = typename Vec<R>::T2;
  constexpr int APW = 64 / LPA;
  constexpr int UNROLL = 4;
  extern __shared__ __align__(16) unsigned char smem[];
  R2 *stab = reinterpret_cast<R2 *>(smem);
  for (int t = threadIdx.x; t < ntypes * ntypes; t += blockDim.x) stab[t] = tab[t];
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int a = wave * APW + lane / LPA;
  const int sub = lane % LPA;
  const bool active = a < n;
  const int aself = active ? a : 0;
  R4 pi;
  pi.x = pi.y = pi.z = pi.w = 0;
  int nn = 0, trow = 0;
  double delta[3] = {0.0, 0.0, 0.0};
  if (active) {
    pi = sorted[a];
    nn = nneigh[a];
    trow = stype[a] * ntypes;
    centre_offset<R>(mol_of, centre, order[a], pi.x, pi.y, pi.z, delta);
  }
  int nmax = nn;
#pragma unroll
  for (int o = 32; o >= LPA; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
  const int nkk = (nmax + LPA - 1) / LPA;
  const unsigned *row = nlist + (size_t)wave * maxn * APW + lane * 4;  // + (kk / 4) * 256 + kk % 4

  double w[3] = {0.0, 0.0, 0.0};
  for (int kk0 = 0; kk0 < nkk; kk0 += UNROLL) {
    unsigned entry[UNROLL];
    R4 pj[UNROLL];
    bool valid[UNROLL];
    int jdx[UNROLL], tj[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) entry[u] = (kk0 + u < nkk) ? row[(size_t)(kk0 >> 2) * 256 + u] : 0u;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      valid[u] = (kk0 + u) * LPA + sub < nn;
      jdx[u] = valid[u] ? (int)((entry[u] & kEntryOffMask) >> 4) : aself;
      pj[u] = sorted[jdx[u]];
      tj[u] = !valid[u] ? 0 : (ntypes <= kEntryTypes ? (int)(entry[u] >> kEntryTypeShift) : stype[jdx[u]]);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const R dx = min_image(pi.x - pj[u].x, c.box[0], c.invbox[0]);
      const R dy = min_image(pi.y - pj[u].y, c.box[1], c.invbox[1]);
      const R dz = min_image(pi.z - pj[u].z, c.box[2], c.invbox[2]);
      const R r2 = norm2(dx, dy, dz);
      const bool hit = valid[u] && (r2 <= c.r2max);
      const R2 ab = stab[trow + tj[u]];
      const R r2s = hit ? r2 : R(1);
      R e4[4] = {0, 0, 0, 0};
      R fs = pair_terms<R, false>(c, r2s, pi.w * pj[u].w, ab.x, ab.y, e4);
      fs = hit ? fs : R(0);
      virial_pair<R>(dx, dy, dz, fs, delta, w);
    }
  }
  block_store3<4>(w[0], w[1], w[2], wpart + 3 * (size_t)blockIdx.x);
}

// allpairs_kernel<R, false> with the force accumulation replaced by the virial's.  grid = (ceil(N / 64), nsplit, replicas), one
// wave per block; boxes[z] = {box[3], 1 / box[3]} (set_boxes); wpart [R][wstride][3], block (x, y) of a replica at y gridDim.x + x
template <typename R>
__global__ __launch_bounds__(64) void virial_allpairs_kernel(int n, const R *__restrict__ pos, const R *__restrict__ qs,
                                                             const int *__restrict__ types, int ntypes,
                                                             const typename Vec<R>::T2 *__restrict__ tab, const int *__restrict__ excl_off,
                                                             const int *__restrict__ excl_idx, PairConsts<R> c, int jchunk,
                                                             const R *__restrict__ boxes, const int *__restrict__ mol_of,
                                                             const double *__restrict__ centre, int nmol, double *__restrict__ wpart,
                                                             int wstride) {
  using R4 = typename Vec<R>::T4;
  __shared__ R4 sj[64];
  __shared__ int st[64];
  const int rep = blockIdx.z;
  pos += (size_t)rep * 3 * n;
  centre += (size_t)rep * 3 * nmol;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c.box[k] = boxes[6 * rep + k];
    c.invbox[k] = boxes[6 * rep + 3 + k];
  }
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  const bool active = i < n;
  const int jbeg = blockIdx.y * jchunk;
  const int jend = min(n, jbeg + jchunk);
  R xi = 0, yi = 0, zi = 0, qi = 0;
  int trow = 0, ebeg = 0, eend = 0;
  double delta[3] = {0.0, 0.0, 0.0};
  if (active) {
    xi = pos[3 * i + 0];
    yi = pos[3 * i + 1];
    zi = pos[3 * i + 2];
    qi = qs[i];
    trow = types[i] * ntypes;
    ebeg = excl_off[i];
    eend = excl_off[i + 1];
    centre_offset<R>(mol_of, centre, i, xi, yi, zi, delta);
  }
  double w[3] = {0.0, 0.0, 0.0};
  for (int j0 = jbeg; j0 < jend; j0 += 64) {
    __syncthreads();
    const int jl = j0 + lane;
    if (jl < jend) {
      R4 v;
      v.x = pos[3 * jl + 0];
      v.y = pos[3 * jl + 1];
      v.z = pos[3 * jl + 2];
      v.w = qs[jl];
      sj[lane] = v;
      st[lane] = types[jl];
    }
    __syncthreads();
    // exclusion mask of this tile for atom i (rows are sorted)
    unsigned long long skip = 0;
    for (int e = ebeg; e < eend; ++e) {
      const int x = excl_idx[e];
      if (x >= j0 + 64) break;
      if (x >= j0) skip |= 1ull << (x - j0);
    }
    if (i >= j0 && i < j0 + 64) skip |= 1ull << (i - j0);
    const int tile = min(64, jend - j0);
    for (int k = 0; k < tile; ++k) {
      const R4 pj = sj[k];
      const R dx = min_image(xi - pj.x, c.box[0], c.invbox[0]);
      const R dy = min_image(yi - pj.y, c.box[1], c.invbox[1]);
      const R dz = min_image(zi - pj.z, c.box[2], c.invbox[2]);
      const R r2 = norm2(dx, dy, dz);
      const bool hit = active && !((skip >> k) & 1ull) && (r2 <= c.r2max);
      if (hit) {
        const typename Vec<R>::T2 ab = tab[trow + st[k]];
        R e4[4] = {0, 0, 0, 0};
        const R fs = pair_terms<R, false>(c, r2, qi * pj.w, ab.x, ab.y, e4);
        virial_pair<R>(dx, dy, dz, fs, delta, w);
      }
    }
  }
  block_store3<1>(w[0], w[1], w[2], wpart + ((size_t)rep * wstride + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3);
}

// one wave per replica: lane l takes the partials l, l + 64, ..., then the butterfly
__global__ __launch_bounds__(64) void virial_fold_kernel(const double *__restrict__ kpart, int kblocks, const double *__restrict__ wpart,
                                                         int wstride, const double *__restrict__ xpart, int xstride,
                                                         const double *__restrict__ boxes, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int r = blockIdx.x;
  double k[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < kblocks; b += 64)
    for (int a = 0; a < 3; ++a) k[a] += kpart[((size_t)r * kblocks + b) * 3 + a];
  for (int b = threadIdx.x; b < wstride; b += 64)
    for (int a = 0; a < 3; ++a) w[a] += wpart[((size_t)r * wstride + b) * 3 + a];
  for (int b = threadIdx.x; b < xstride; b += 64)
    for (int a = 0; a < 3; ++a) w[a] += xpart[((size_t)r * xstride + b) * 3 + a];
  for (int a = 0; a < 3; ++a) k[a] = wave_sum(k[a]), w[a] = wave_sum(w[a]);
  if (threadIdx.x == 0) virial_finish(k, w, boxes + 3 * (size_t)r, out + 8 * (size_t)r);
}

template <typename T>
int upload(DevBuf &b, const T *src, size_t count) {
  TMD_TRY(b.ensure(std::max<size_t>(sizeof(T) * count, 16)));
  if (count) TMD_HIP(hipMemcpy(b.p, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return 0;
}

// a molecule without mass has no centre: refused where masses are first seen (one read-back per mass array)
int check_masses(tmdhip_ctx *ctx, VirialState *S, const void *mass_dev, hipStream_t st) {
  if (S->mass_checked == mass_dev) return 0;
  std::vector<char> host((size_t)ctx->real_size * S->natoms);
  TMD_HIP(hipMemcpyAsync(host.data(), mass_dev, host.size(), hipMemcpyDeviceToHost, st));
  TMD_HIP(hipStreamSynchronize(st));
  for (int m = 0; m < S->nmol; ++m) {
    double sum = 0.0;
    for (int k = S->off_h[m]; k < S->off_h[m + 1]; ++k) {
      const int a = S->mem_h[k];
      sum += ctx->d.dtype == TMDHIP_F32 ? (double)((const float *)host.data())[a] : ((const double *)host.data())[a];
    }
    if (!(sum > 0.0)) return fail("tmdhip_pressure: molecule " + std::to_string(m) + " has no mass (its centre is undefined)");
  }
  S->mass_checked = mass_dev;
  return 0;
}

// the j split of launch_allpairs (pair_generic.hip)
void allpairs_split(int n, int nrep, int &nb, int &nsplit, int &jchunk) {
  nb = (n + 63) / 64;
  const double pairs = (double)n * (double)n * (double)nrep;
  const int want_waves = (int)std::min(4096.0, std::max(1024.0, pairs / 512.0));
  nsplit = std::max(1, std::min((n + 15) / 16, want_waves / std::max(nb * nrep, 1)));
  jchunk = ((n + nsplit - 1) / nsplit + 15) / 16 * 16;
  nsplit = (n + jchunk - 1) / jchunk;
}

template <typename R>
int launch_list(tmdhip_ctx *ctx, VirialState *S, Replica &rp, const PairConsts<R> &c, const double *centre, double *wpart, hipStream_t st) {
  using R4 = typename Vec<R>::T4;
  using R2 = typename Vec<R>::T2;
  const int n = ctx->d.natoms;
  const int waves = (n + rp.lg.apw - 1) / rp.lg.apw;
  const int blocks = (waves + 3) / 4;
  const size_t shmem = (size_t)ctx->d.ntypes * ctx->d.ntypes * sizeof(R2);
#define TMD_LAUNCH(L)                                                                                                             \
  hipLaunchKernelGGL((virial_list_kernel<R, L>), dim3(blocks), dim3(256), shmem, st, n, rp.sorted.as<R4>(), rp.stype.as<int>(),   \
                     rp.order.as<int>(), ctx->d.ntypes, ctx->tab.as<R2>(), rp.nlist.as<unsigned>(), rp.nneigh.as<int>(), rp.lg.maxn, \
                     c, S->mol_of.as<int>(), centre, wpart)
  switch (rp.lg.lpa) {
    case 1: TMD_LAUNCH(1); break;
    case 2: TMD_LAUNCH(2); break;
    case 4: TMD_LAUNCH(4); break;
    case 8: TMD_LAUNCH(8); break;
    case 16: TMD_LAUNCH(16); break;
    case 32: TMD_LAUNCH(32); break;
    default: TMD_LAUNCH(64); break;
  }
#undef TMD_LAUNCH
  TMD_HIP(hipGetLastError());
  return 0;
}

inline int list_blocks(const tmdhip_ctx *ctx, const Replica &rp) {
  const int waves = (ctx->d.natoms + rp.lg.apw - 1) / rp.lg.apw;
  return (waves + 3) / 4;
}

template <typename R>
int pressure(tmdhip_ctx *ctx, VirialState *S, const void *pos_dev, const void *vel_dev, const void *mass_dev, const double *box_host,
             double *out_host, hipStream_t st) {
  using R2 = typename Vec<R>::T2;
  const int n = ctx->d.natoms, nrep = (int)ctx->rep.size(), nmol = S->nmol;
  const size_t stride = (size_t)n * 3;
  const R *pos = (const R *)pos_dev;
  TMD_TRY(S->centre.ensure(sizeof(double) * 3 * (size_t)nmol * nrep));
  TMD_TRY(S->kpart.ensure(sizeof(double) * 3 * (size_t)S->kblocks * nrep));
  TMD_TRY(S->out.ensure(sizeof(double) * 8 * (size_t)nrep));
  TMD_TRY(S->boxes.ensure(sizeof(double) * 3 * (size_t)nrep));
  TMD_HIP(hipMemcpyAsync(S->boxes.p, box_host, sizeof(double) * 3 * (size_t)nrep, hipMemcpyHostToDevice, st));  // (pageable: staged before the call returns)

  const int small_blocks = (nmol + kThreads - 1) / kThreads;
  hipLaunchKernelGGL((mol_centre_kernel<R>), dim3((unsigned)small_blocks, (unsigned)nrep), dim3(kThreads), 0, st, n, nmol, S->off.as<int>(),
                     S->mem.as<int>(), S->big.as<int>(), pos, (const R *)vel_dev, (const R *)mass_dev, S->centre.as<double>(),
                     S->kpart.as<double>(), S->kblocks, small_blocks, 0);
  if (S->nbig)
    hipLaunchKernelGGL((mol_centre_kernel<R>), dim3((unsigned)S->nbig, (unsigned)nrep), dim3(kWave), 0, st, n, nmol, S->off.as<int>(),
                       S->mem.as<int>(), S->big.as<int>(), pos, (const R *)vel_dev, (const R *)mass_dev, S->centre.as<double>(),
                       S->kpart.as<double>(), S->kblocks, small_blocks, 1);
  TMD_HIP(hipGetLastError());

  int wstride = 1;
  bool lists = false;
  if (ctx->d.terms != 0 && ctx->algorithm == TMDHIP_ALGO_CELLLIST) {
    // the list of every replica is brought up to date exactly as an evaluation would (displacement test, rebuild chain, the step
    // counter); the pair launch is ours
    lists = true;
    std::vector<ListOnlyOut> lo(nrep);
    for (int r = 0; r < nrep && lists; ++r) {
      Replica &rp = ctx->rep[r];
      const int rc = compute_list<R>(ctx, rp, pos + r * stride, box_host + 3 * r, nullptr, nullptr, kListOnly, st, nullptr, &lo[r]);
      if (rc == kFallbackAllPairs) {
        ctx->algorithm = TMDHIP_ALGO_ALLPAIRS;  // AUTO and the box holds fewer than 3 cells per edge (as tmdhip_compute_nonbonded)
        lists = false;
      } else if (rc != 0) {
        return rc;
      }
      rp.seq_valid = false;  // (as a plain evaluation leaves it: the MD loop's pacing must not read an older report as current)
    }
    if (lists) {
      for (int r = 0; r < nrep; ++r) wstride = std::max(wstride, list_blocks(ctx, ctx->rep[r]));
      TMD_TRY(S->wpart.ensure(sizeof(double) * 3 * (size_t)wstride * nrep));
      TMD_HIP(hipMemsetAsync(S->wpart.p, 0, sizeof(double) * 3 * (size_t)wstride * nrep, st));  // (replicas with fewer blocks)
      for (int r = 0; r < nrep; ++r)
        TMD_TRY(launch_list<R>(ctx, S, ctx->rep[r], make_consts<R>(ctx, box_host + 3 * r), S->centre.as<double>() + (size_t)r * 3 * nmol,
                               S->wpart.as<double>() + (size_t)r * 3 * wstride, st));
    }
  }
  if (ctx->d.terms != 0 && !lists) {
    int nb, nsplit, jchunk;
    allpairs_split(n, nrep, nb, nsplit, jchunk);
    wstride = nb * nsplit;
    TMD_TRY(S->wpart.ensure(sizeof(double) * 3 * (size_t)wstride * nrep));
    const R *boxes = (const R *)set_boxes(ctx, box_host, st);
    if (!boxes) return fail("tmdhip_pressure: could not upload the replica boxes");
    const PairConsts<R> c = make_consts<R>(ctx, box_host);
    hipLaunchKernelGGL((virial_allpairs_kernel<R>), dim3((unsigned)nb, (unsigned)nsplit, (unsigned)nrep), dim3(64), 0, st, n, pos,
                       ctx->qs.as<R>(), ctx->types.as<int>(), ctx->d.ntypes, ctx->tab.as<R2>(), ctx->excl_off.as<int>(),
                       ctx->excl_idx.as<int>(), c, jchunk, boxes, S->mol_of.as<int>(), S->centre.as<double>(), nmol,
                       S->wpart.as<double>(), wstride);
    TMD_HIP(hipGetLastError());
  }
  if (ctx->d.terms == 0) {
    TMD_TRY(S->wpart.ensure(sizeof(double) * 3 * (size_t)nrep));
    TMD_HIP(hipMemsetAsync(S->wpart.p, 0, sizeof(double) * 3 * (size_t)nrep, st));
  }
  const int xstride = pme_virial_partials(ctx);  // (0 without PME)
  if (xstride) {
    TMD_TRY(S->xpart.ensure(sizeof(double) * 3 * (size_t)xstride * nrep));
    for (int r = 0; r < nrep; ++r)
      TMD_TRY(pme_virial<R>(ctx, r, pos + r * stride, box_host + 3 * r, S->mol_of.as<int>(), S->centre.as<double>() + (size_t)r * 3 * nmol,
                            S->xpart.as<double>() + (size_t)r * 3 * xstride, st));
  }
  hipLaunchKernelGGL(virial_fold_kernel, dim3((unsigned)nrep), dim3(64), 0, st, S->kpart.as<double>(), S->kblocks, S->wpart.as<double>(),
                     wstride, S->xpart.as<double>(), xstride, S->boxes.as<double>(), S->out.as<double>());
  TMD_HIP(hipGetLastError());
  TMD_HIP(hipMemcpyAsync(out_host, S->out.p, sizeof(double) * 8 * (size_t)nrep, hipMemcpyDeviceToHost, st));
  std::vector<int> hf;
  if (lists) {
    hf.resize((size_t)F_COUNT * nrep);
    for (int r = 0; r < nrep; ++r)
      TMD_HIP(hipMemcpyAsync(hf.data() + (size_t)r * F_COUNT, ctx->rep[r].flags.p, sizeof(int) * F_COUNT, hipMemcpyDeviceToHost, st));
  }
  TMD_HIP(hipStreamSynchronize(st));
  int verdict = 0;
  if (lists)
    for (int r = 0; r < nrep; ++r)
      if (ctx->rep[r].have_list) {
        const int rc = judge_flags(ctx, ctx->rep[r], hf.data() + (size_t)r * F_COUNT, st);
        if (rc < 0) return rc;
        verdict |= rc;
      }
  return verdict;
}

}  // namespace

namespace tmd {

void virial_release(tmdhip_ctx *ctx) {
  VirialState *S = (VirialState *)ctx->virial;
  if (!S) return;
  S->release();
  delete S;
  ctx->virial = nullptr;
}

}  // namespace tmd

extern "C" {

int tmdhip_set_molecules(tmdhip_ctx *ctx, const tmdhip_molecule_desc *desc) {
  if (!ctx || !desc) return fail("tmdhip_set_molecules: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_molecule_desc)) return fail("tmdhip_set_molecules: tmdhip_molecule_desc size mismatch (ABI)");
  const int n = ctx->d.natoms;
  if (ctx->nactive < n) return fail("tmdhip_set_molecules: not for a context with passive atoms (a brick of the domain decomposition)");
  std::vector<int32_t> mol_of;
  const std::string why = virial_validate_molecules(n, desc->nmol, desc->offsets_host, desc->members_host, mol_of);
  if (!why.empty()) return fail("tmdhip_set_molecules: " + why);
  TMD_HIP(hipDeviceSynchronize());  // (a launch that reads the old tables may still be in flight)
  VirialState *S = (VirialState *)ctx->virial;
  if (!S) ctx->virial = S = new VirialState;
  S->nmol = desc->nmol;
  S->natoms = n;
  S->off_h.assign(desc->offsets_host, desc->offsets_host + desc->nmol + 1);
  S->mem_h.assign(desc->members_host, desc->members_host + n);
  S->mass_checked = nullptr;
  std::vector<int32_t> big;
  for (int m = 0; m < S->nmol; ++m)
    if (S->off_h[m + 1] - S->off_h[m] > kBigMol) big.push_back(m);
  S->nbig = (int)big.size();
  S->kblocks = (S->nmol + kThreads - 1) / kThreads + S->nbig;
  int rc = upload(S->off, S->off_h.data(), S->off_h.size());
  if (rc == 0) rc = upload(S->mem, S->mem_h.data(), S->mem_h.size());
  if (rc == 0) rc = upload(S->mol_of, mol_of.data(), mol_of.size());
  if (rc == 0) rc = upload(S->big, big.data(), big.size());
  if (rc != 0) {
    virial_release(ctx);
    return rc;
  }
  TMD_HIP(hipDeviceSynchronize());
  return 0;
}

int tmdhip_pressure(tmdhip_ctx *ctx, const void *pos_dev, const void *vel_dev, const void *mass_dev, const double *box_host,
                    double *out_host, void *stream) {
  if (!ctx || !pos_dev || !mass_dev || !box_host || !out_host) return fail("tmdhip_pressure: null argument");
  const int n = ctx->d.natoms, nrep = (int)ctx->rep.size();
  if (ctx->nactive < n) return fail("tmdhip_pressure: not for a context with passive atoms (a brick of the domain decomposition)");
  VirialState *S = (VirialState *)ctx->virial;
  if (!S || S->natoms != n) return fail("tmdhip_pressure: the molecules are not set (tmdhip_set_molecules)");
  for (int k = 0; k < 3 * nrep; ++k)
    if (!(box_host[k] > 0.0) || !std::isfinite(box_host[k])) return fail("tmdhip_pressure: every box edge must be positive (a pressure needs a volume)");
  hipStream_t st = (hipStream_t)stream;
  TMD_TRY(check_masses(ctx, S, mass_dev, st));
  return ctx->d.dtype == TMDHIP_F32 ? pressure<float>(ctx, S, pos_dev, vel_dev, mass_dev, box_host, out_host, st)
                                    : pressure<double>(ctx, S, pos_dev, vel_dev, mass_dev, box_host, out_host, st);
}

}  // extern "C"
