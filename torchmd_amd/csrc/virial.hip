// Instantaneous pressure: the molecular virial of the nonbonded force field and the kinetic term of the molecules' centres, for
// gfx950 (tmdhip_set_molecules, tmdhip_pressure; the per-pair arithmetic: virial_math.h).
//
//   P_aa V = sum_I M_I V_I,a^2 + W_aa,   W_aa = 1/2 sum_i sum_{j in list(i)} d_ij,a f_ij,a - sum_i delta_i,a F_i,a
// with R_I / V_I the mass-weighted centre of molecule I and its velocity and delta_i = r_i - R_I(i).  Under a rigid displacement of
// whole molecules the bonded terms, the constraint forces and every other intramolecular force do no work, so none of them
// appears; molecules must be whole (no minimum image inside a molecule: the barostat's contract).
//
// Separate launches between two tmdhip_md_run calls, like a plain evaluation.  The pair kernels walk the pair set with the
// functions the force kernels use (pair_walk.h), at the launch geometry the force launches use (list_blocks, allpairs_split).
//   mol_centre_kernel      one thread per molecule of <= 64 atoms (one wave per larger one: a second launch, only when such
//                          molecules exist), blockIdx.y = replica: R_I in double, per-block partials of sum M_I V_I,a^2
//   virial_list_kernel     walk_list_rows, as list_pair_kernel<R, false, LPA, 0>: every lane adds f_a (d_a / 2 - delta_i,a)
//                          pair by pair in double; the block's three partials
//   virial_allpairs_kernel walk_allpairs_tiles, as allpairs_kernel: all-pairs contexts and cell-list contexts that fell back
//   pme.hip: pme_virial    PME contexts: the chain of pme_apply (pme_forward / pme_inverse) with the modes' W^rec from
//                          pme_conv_virial_kernel, -delta_i . F^rec_i from the force kernel into a scratch array, and the
//                          neutralising background, as partials of their own
//   virial_fold_kernel     one wave per replica folds the partials; writes
//                          double [R][8] = (sum M V^2 x, y, z; W x, y, z; V; P)
// Fixed-order sum (reduce.h), the wave sums meet pairwise: two calls on the same state give the same bits.
// The pair kernels are bound like the generic list kernel (gather latency + pair_terms); everything else is a few
// microseconds of launch.
#include "pair_walk.h"
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
  double k[3] = {0, 0, 0};
  if (work) {
    double *c = centre + ((size_t)r * nmol + g) * 3;
    c[0] = sx / sm, c[1] = sy / sm, c[2] = sz / sm;
    // M V_a^2 = (sum m v_a)^2 / M
    k[0] = px * px / sm, k[1] = py * py / sm, k[2] = pz * pz / sm;
  }
  double *dst = kpart + ((size_t)r * kblocks + (big_pass ? small_blocks + blockIdx.x : blockIdx.x)) * 3;
  if (big_pass) {  // (lane 0 alone holds the molecule's term)
    if (threadIdx.x == 0) dst[0] = k[0], dst[1] = k[1], dst[2] = k[2];
  } else {
    block_sums<kThreads / 64, Meet::Pairwise>(k, dst);
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

// list_pair_kernel<R, false, LPA, 0>'s walk (pair_walk.h) with the virial's accumulation; wpart: this replica's [blocks][3]
template <typename R, int LPA>
__global__ __launch_bounds__(256) void virial_list_kernel(int n, const typename Vec<R>::T4 *__restrict__ sorted, const int *__restrict__ stype,
                                                          const int *__restrict__ order, int ntypes,
                                                          const typename Vec<R>::T2 *__restrict__ tab, const unsigned *__restrict__ nlist,
                                                          const int *__restrict__ nneigh, int maxn, PairConsts<R> c,
                                                          const int *__restrict__ mol_of, const double *__restrict__ centre,
                                                          double *__restrict__ wpart) {
  double delta[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  walk_list_rows<R, LPA>(
      n, sorted, stype, ntypes, tab, nlist, nneigh, maxn, c,
      [&](int a, const typename Vec<R>::T4 &pi) { centre_offset<R>(mol_of, centre, order[a], pi.x, pi.y, pi.z, delta); },
      [&](R dx, R dy, R dz, R r2s, bool hit, R qq, typename Vec<R>::T2 ab) {
        R e4[4] = {0, 0, 0, 0};
        R fs = pair_terms<R, false>(c, r2s, qq, ab.x, ab.y, e4);
        fs = hit ? fs : R(0);
        virial_pair<R>(dx, dy, dz, fs, delta, w);
      });
  block_sums<4, Meet::Pairwise>(w, wpart + 3 * (size_t)blockIdx.x);
}

// allpairs_kernel<R, false>'s walk (pair_walk.h) with the virial's accumulation.  grid = (nb, nsplit, replicas) of allpairs_split,
// one wave per block; boxes[z] = {box[3], 1 / box[3]} (set_boxes); wpart [R][nb nsplit][3], block (x, y) of a replica at y nb + x
template <typename R>
__global__ __launch_bounds__(64) void virial_allpairs_kernel(int n, const R *__restrict__ pos, const R *__restrict__ qs,
                                                             const int *__restrict__ types, int ntypes,
                                                             const typename Vec<R>::T2 *__restrict__ tab, const int *__restrict__ excl_off,
                                                             const int *__restrict__ excl_idx, PairConsts<R> c, int jchunk,
                                                             const R *__restrict__ boxes, const int *__restrict__ mol_of,
                                                             const double *__restrict__ centre, int nmol, double *__restrict__ wpart) {
  const int rep = blockIdx.z;
  pos += (size_t)rep * 3 * n;
  centre += (size_t)rep * 3 * nmol;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c.box[k] = boxes[6 * rep + k];
    c.invbox[k] = boxes[6 * rep + 3 + k];
  }
  const int i = blockIdx.x * 64 + threadIdx.x;
  double delta[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  if (i < n) centre_offset<R>(mol_of, centre, i, pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2], delta);
  walk_allpairs_tiles<R>(n, pos, qs, types, ntypes, tab, excl_off, excl_idx, c, jchunk,
                         [&](R dx, R dy, R dz, R r2, R qq, typename Vec<R>::T2 ab, int) {
                           R e4[4] = {0, 0, 0, 0};
                           const R fs = pair_terms<R, false>(c, r2, qq, ab.x, ab.y, e4);
                           virial_pair<R>(dx, dy, dz, fs, delta, w);
                         });
  const size_t slot = ((size_t)rep * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  block_sums<1, Meet::Pairwise>(w, wpart + 3 * slot);
}

// one wave per replica; the pair rows and the PME rows share one accumulator (the PME rows behind the pair rows, lane by lane)
__global__ __launch_bounds__(64) void virial_fold_kernel(const double *__restrict__ kpart, int kblocks, const double *__restrict__ wpart,
                                                         int wstride, const double *__restrict__ xpart, int xstride,
                                                         const double *__restrict__ boxes, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int r = blockIdx.x;
  double k[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  fold_into(k, kpart + (size_t)r * kblocks * 3, kblocks);
  fold_into(w, wpart + (size_t)r * wstride * 3, wstride);
  fold_into(w, xpart + (size_t)r * xstride * 3, xstride);
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

template <typename R>
int launch_list(tmdhip_ctx *ctx, VirialState *S, Replica &rp, const PairConsts<R> &c, const double *centre, double *wpart, hipStream_t st) {
  using R4 = typename Vec<R>::T4;
  using R2 = typename Vec<R>::T2;
  const size_t shmem = (size_t)ctx->d.ntypes * ctx->d.ntypes * sizeof(R2);
  dispatch_lpa(rp.lg.lpa, [&](auto lpa) {
    hipLaunchKernelGGL((virial_list_kernel<R, decltype(lpa)::value>), dim3(list_blocks(ctx, rp)), dim3(256), shmem, st, ctx->d.natoms,
                       rp.sorted.as<R4>(), rp.stype.as<int>(), rp.order.as<int>(), ctx->d.ntypes, ctx->tab.as<R2>(),
                       rp.nlist.as<unsigned>(), rp.nneigh.as<int>(), rp.lg.maxn, c, S->mol_of.as<int>(), centre, wpart);
  });
  TMD_HIP(hipGetLastError());
  return 0;
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
                       S->wpart.as<double>());
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
