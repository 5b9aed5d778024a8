// The MD loop of the nonbonded engine for gfx950 (MI355X): fused MD-step kernels and tmdhip_md_run / _restore, which
// enqueue whole batches of steps from C.  (The constrained step: md_cons.hip; the reports to the host: md_observe.hip.)
//
// Reference semantics: torchmd/integrator.py:61-74 (_first_VV, _second_VV, langevin) in the order of
// Integrator.step (integrator.py:112-125): first_VV(old F) -> compute -> langevin -> second_VV(new F).
#include "engine.h"
#include "md_step.h"

namespace tmd {

template <typename R, bool SECOND, bool LANGEVIN, bool FIRST, bool CHECK>
__global__ void md_step_kernel(MdStepArgs<R> s, PairConsts<R> c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (CHECK && i == 0) list_check_clear(s.chk.flags, s.chk.parity);
  if (i >= s.n) return;
  // replica batch (all-pairs systems, never with CHECK): blockIdx.y = replica
  const size_t off = CHECK ? 0 : (size_t)blockIdx.y * 3 * s.n;
  const uint64_t row0 = s.row0 + (CHECK ? 0 : (uint64_t)blockIdx.y * (uint64_t)s.n);
  const R none[3] = {0, 0, 0};
  const AtomIn<R> x = md_load_atom<R, SECOND, LANGEVIN, FIRST, CHECK>(s, i, off);
  if constexpr (FIRST && !SECOND && CHECK) {
    if (s.snap_pos) {  // the state at the entry of the call (tmdhip_md_restore), from the registers just loaded
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s.snap_pos[3 * i + k] = x.p[k];
        s.snap_vel[3 * i + k] = x.v[k];
        s.snap_f[3 * i + k] = x.f[k];
      }
      if (s.zero && i < s.nzero) s.zero[i] = 0.0;
    }
  }
  md_step_atom<R, SECOND, LANGEVIN, FIRST, CHECK>(s, c, i, off, row0, x, none, false);
}

// Interior steps of an MD run: the bonded force of the previous step's positions is evaluated HERE
// instead of by a bonded kernel of its own (one launch and one read-modify-write pass over `forces` less
// per step; bit-identical to the separate kernels: the same device functions in the same order, added to
// the stored pair force before the division by the mass).  Partner positions must be the undrifted ones,
// so the step reads pos_in and writes pos_out (two buffers).  Light topologies only (thread per atom,
// per-atom records): for proteins a wave-per-atom variant with lane 0 integrating was measured slower than
// the separate bonded_wave_kernel (alanine dipeptide 47 vs 42.5 us/step: the two phases serialise inside
// each wave).  Without CHECK (all-pairs systems) blockIdx.y is the replica.
template <typename R, bool LANGEVIN, bool CHECK>
__global__ __launch_bounds__(256) void md_step_bonded_kernel(MdStepArgs<R> s, PairConsts<R> c, BondedArgs<R> A,
                                                             const R *__restrict__ boxes) {
  if (CHECK && blockIdx.x == 0 && threadIdx.x == 0) list_check_clear(s.chk.flags, s.chk.parity);
  const int rep = CHECK ? 0 : (int)blockIdx.y;
  const size_t off = (size_t)rep * 3 * s.n;
  const uint64_t row0 = s.row0 + (uint64_t)rep * (uint64_t)s.n;
  if (!CHECK && boxes) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      A.b.box[k] = boxes[6 * rep + k];
      A.b.invbox[k] = boxes[6 * rep + 3 + k];
    }
  }
  const R *pos = s.pos_in + off;
  R fx = 0, fy = 0, fz = 0;
  double e[TMDHIP_NENERGY] = {0, 0, 0, 0, 0, 0, 0, 0};  // energies are not wanted on interior steps (dead)
  // A block of 256 threads = 64 atoms.  Bonded records: wave w evaluates slots w, w + 4, ... of all 64 atoms
  // (lane = atom), so that the lanes of a wave work on the same KIND of record wherever the atoms' record lists
  // look alike — water: waves 0 and 1 evaluate a bond for every atom, wave 2 an angle, wave 3 has nothing to do —
  // instead of four adjacent lanes per atom running the bond and the angle code one after the other (kernel
  // 8.95 -> 8.15 us at C3; the rest is memory round trips).  The per-slot partial forces meet in LDS and are
  // added in the order of eval_atom_quad's butterfly, (p0 + p1) + (p2 + p3): bit-identical to the separate
  // bonded kernel.  The update itself (noise, kicks, drift) runs one atom per lane on the block's first wave,
  // which issues the loads of its 64 atoms before the bonded part so that they are in flight meanwhile.
  __shared__ R s_part[kQuad][3][64];
  const int a0 = blockIdx.x * 64;
  const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int mine = a0 + lane;  // this lane's atom: its slots w, w + 4, ... here, its update on the first wave
  const bool integrates = w == 0 && mine < s.n;
  AtomIn<R> x{};
  if (integrates) x = md_load_atom<R, true, LANGEVIN, true, CHECK>(s, mine, off);
  if (mine < s.n) {
    const AtomRec<R> *rec = A.arec + (size_t)mine * A.arec_stride;
    for (int k = w; k < A.arec_stride; k += kQuad) {
      const AtomRec<R> r = rec[k];
      if (r.ent == kNoRec) break;  // records are packed from the front
      eval_rec<R>(A, pos, mine, r, fx, fy, fz, e);
    }
  }
  s_part[w][0][lane] = fx;
  s_part[w][1][lane] = fy;
  s_part[w][2][lane] = fz;
  __syncthreads();
  if (!integrates) return;
  R fb[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) fb[k] = (s_part[0][k][lane] + s_part[1][k][lane]) + (s_part[2][k][lane] + s_part[3][k][lane]);
  md_step_atom<R, true, LANGEVIN, true, CHECK>(s, c, mine, off, row0, x, fb, true);
}

// state at the entry of an MD batch (positions, velocities, forces) in one launch; n4 = 16-byte words per array
__global__ void snapshot3_kernel(size_t n4, const uint4 *__restrict__ a, const uint4 *__restrict__ b,
                                 const uint4 *__restrict__ c, uint4 *__restrict__ out, double *__restrict__ zero,
                                 int nzero) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (zero && i < (size_t)nzero) zero[i] = 0.0;  // the call's energy buffer (one fill launch less per call)
  if (i >= n4) return;
  out[i] = a[i];
  out[n4 + i] = b[i];
  out[2 * n4 + i] = c[i];
}
// can a kernel (this one, or the first integrator kernel of the call) take the snapshot?  16-byte words throughout
inline bool snapshot_by_kernel(const tmdhip_md_desc *d, size_t bytes) {
  return ((uintptr_t)d->pos_dev | (uintptr_t)d->vel_dev | (uintptr_t)d->forces_dev) % 16 == 0 && bytes % 16 == 0;
}

template <typename R, bool SECOND, bool LANGEVIN, bool FIRST>
void launch_md_step(const MdStepArgs<R> &a, const PairConsts<R> &c, bool check, hipStream_t st, int nrep = 1) {
  const dim3 grid((a.n + 255) / 256, check ? 1 : nrep), block(256);
  if (check)
    hipLaunchKernelGGL((md_step_kernel<R, SECOND, LANGEVIN, FIRST, true>), grid, block, 0, st, a, c);
  else
    hipLaunchKernelGGL((md_step_kernel<R, SECOND, LANGEVIN, FIRST, false>), grid, block, 0, st, a, c);
}

template <typename R>
void launch_md_step_bonded(const MdStepArgs<R> &a, const PairConsts<R> &c, const BondedArgs<R> &A, bool langevin,
                           bool check, const R *boxes, int nrep, hipStream_t st) {
  const dim3 grid((kQuad * a.n + 255) / 256, check ? 1 : nrep), block(256);
#define TMD_MSB(L, C) hipLaunchKernelGGL((md_step_bonded_kernel<R, L, C>), grid, block, 0, st, a, c, A, boxes)
  if (langevin && check) TMD_MSB(true, true);
  else if (langevin) TMD_MSB(true, false);
  else if (check) TMD_MSB(false, true);
  else TMD_MSB(false, false);
#undef TMD_MSB
}

// ---- chain skipping (ListCheck) --------------------------------------------------------------------
constexpr int64_t kChainSkipMinEntries = 1'000'000;  // list slots from which the host paces itself behind the device.  (Round 2 gated this
                                                    // at 2e7 "because shorter pair kernels cannot hide the host"; measured in round 3 with the gate
                                                    // open, water boxes, us per MD step: 5 184 atoms 23.9 -> 22.6, 12 288 atoms 34.6 -> 28.6,
                                                    // 24 000 atoms 42.4 -> 36.8, bit-identical trajectories.)

// spin until the device has published sequence number `target` (wrap-around safe); false after 0.2 s
bool wait_published(volatile unsigned *hp, unsigned target) {
  if ((int)(hp[0] - target) >= 0) return true;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1;; ++spins) {
    if ((int)(hp[0] - target) >= 0) return true;
    __builtin_ia32_pause();
    if ((spins & 4095u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) return false;
  }
}

// a list exists and was built for this box
inline bool list_matches_box(const Replica &rp, const double *box) {
  return rp.have_list && box[0] == rp.box[0] && box[1] == rp.box[1] && box[2] == rp.box[2];
}

template <typename R>
int pace_behind_device(Replica &rp, ListCheck<R> &chk, bool follows, double near_frac, bool &timed_out, bool &skip_chain) {
  if (!rp.hostpub) {
    TMD_HIP(hipHostMalloc((void **)&rp.hostpub, 8 * sizeof(unsigned), hipHostMallocMapped));
    for (int w = 0; w < 8; ++w) rp.hostpub[w] = 0u;
    rp.seq = 0;
    rp.seq_valid = false;
  }
  if (rp.seq_valid && follows && !timed_out && !wait_published(rp.hostpub, rp.seq)) timed_out = true;
  const PaceStep p = pace_decide(rp.hostpub, rp.seq, rp.seq_valid, follows, timed_out, rp.prev_skipped);
  skip_chain = rp.prev_skipped = p.skip_chain;
  rp.seq = p.seq;
  chk.near_host = rp.hostpub + 1 + (rp.seq & 1u);
  chk.seq = rp.seq;
  chk.near_frac2 = (R)(near_frac * near_frac);
  chk.skipped = skip_chain ? 1 : 0;
  rp.seq_valid = true;
  rp.pub_ptr = rp.hostpub;
  rp.pub_val = rp.seq;
  return 0;
}
template int pace_behind_device<float>(Replica &, ListCheck<float> &, bool, double, bool &, bool &);
template int pace_behind_device<double>(Replica &, ListCheck<double> &, bool, double, bool &, bool &);

// the static arguments of the fused step travel as a kernel argument (stream-ordered, no pinned staging, no host wait)
template <typename R>
__global__ void fused_upload_kernel(FusedStaticT<R> v, FusedStaticT<R> *dst) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}

template <typename R>
int upload_fused_static(Replica &rp, const FusedStaticT<R> &now, hipStream_t st) {
  static_assert(sizeof(FusedStaticT<R>) <= sizeof(rp.fused_host), "Replica::fused_host holds either precision");
  TMD_TRY(rp.fused_dev.ensure(sizeof(FusedStaticT<double>)));
  if (!rp.fused_host_valid || std::memcmp(rp.fused_host, &now, sizeof(now)) != 0) {
    hipLaunchKernelGGL((fused_upload_kernel<R>), dim3(1), dim3(64), 0, st, now, rp.fused_dev.as<FusedStaticT<R>>());
    TMD_HIP(hipGetLastError());
    std::memcpy(rp.fused_host, &now, sizeof(now));
    rp.fused_host_valid = true;
  }
  return 0;
}
template int upload_fused_static<float>(Replica &, const FusedStaticT<float> &, hipStream_t);
template int upload_fused_static<double>(Replica &, const FusedStaticT<double> &, hipStream_t);

template <typename R>
void fused_static_common(FusedStaticT<R> &now, int n, R *vel, const R *mass, const R *vcoeff, double dt, R gamma, uint64_t seed,
                         uint64_t row0, const R *qs, const int *inv, const ListCheck<R> &chk, double near_frac) {
  std::memset(&now, 0, sizeof(now));
  now.s.n = n;
  now.s.vel = vel;
  now.s.mass = mass;
  now.s.vcoeff = vcoeff;
  now.s.dt = (R)dt;
  now.s.half_dt = (R)(0.5 * dt);
  now.s.gamma = gamma;
  now.s.seed = seed;
  now.s.row0 = row0;
  now.s.qs = qs;
  now.s.inv = inv;
  now.s.chk.ref = chk.ref;
  now.s.chk.hard2 = chk.hard2;
  now.s.chk.hs2 = chk.hs2;
  now.s.chk.flags = chk.flags;
  now.s.chk.near_frac2 = (R)(near_frac * near_frac);
  now.s.chk.ext = chk.ext;
}
template void fused_static_common<float>(FusedStaticT<float> &, int, float *, const float *, const float *, double, float, uint64_t, uint64_t,
                                         const float *, const int *, const ListCheck<float> &, double);
template void fused_static_common<double>(FusedStaticT<double> &, int, double *, const double *, const double *, double, double, uint64_t,
                                          uint64_t, const double *, const int *, const ListCheck<double> &, double);

template <typename R>
int fused_launch_common(Replica &rp, const FusedStaticT<R> &now, bool langevin, const R *pos_in, R *pos_out, uint64_t noise_step,
                        bool paced, FusedLaunchT<R> &fl, hipStream_t st) {
  TMD_TRY(upload_fused_static(rp, now, st));
  fl.fst = rp.fused_dev.as<FusedStaticT<R>>();
  fl.langevin = langevin;
  fl.step.pos_in = pos_in;
  fl.step.pos_out = pos_out;
  fl.step.sorted_out = rp.sorted_alt.as<typename Vec<R>::T4>();
  fl.step.noise_step = noise_step;
  fl.step.bonded = now.has_bonded;
  if (paced) {
    fl.step.seq = next_seq(rp.seq);
    fl.step.near_host = rp.hostpub + 1 + (fl.step.seq & 1u);
  }
  return 0;
}
template int fused_launch_common<float>(Replica &, const FusedStaticT<float> &, bool, const float *, float *, uint64_t, bool,
                                        FusedLaunchT<float> &, hipStream_t);
template int fused_launch_common<double>(Replica &, const FusedStaticT<double> &, bool, const double *, double *, uint64_t, bool,
                                         FusedLaunchT<double> &, hipStream_t);

int begin_fused_launch(Replica &rp, int n, hipStream_t st, unsigned &gen) {
  if (rp.fsort.bytes < sizeof(float4) * (size_t)n) {
    TMD_TRY(rp.fsort.ensure(sizeof(float4) * (size_t)n));
    TMD_HIP(hipMemsetAsync(rp.fsort.p, 0, rp.fsort.bytes, st));
    rp.fused_gen = 0;
  }
  if (rp.fused_gen == 0)
    if (const char *e = std::getenv("TMDHIP_DEBUG_FUSED_GEN0")) rp.fused_gen = (unsigned)std::strtoul(e, nullptr, 0);
  gen = rp.fused_gen = next_seq(rp.fused_gen);
  rp.fused_launches++;
  return 0;
}

// can the pair launch of this replica integrate the next step itself?  (lean fp32 kernel, 4 .. 64 lanes per atom: a pair
// block's atoms fit one wave of a step block.  fp64: built in round 4, bit-identical and slower — 151 against 124.5 us
// per step at C3, no partial last round of pair blocks for the step blocks to hide in — and removed in round 5.)
template <typename R>
bool fused_step_possible(const tmdhip_ctx *ctx, const Replica &rp, const PairConsts<R> &c) {
  if (std::is_same<R, double>::value) return false;
  const char *e = std::getenv("TMDHIP_FUSED_STEP");  // (read per call: tests switch it within a process)
  if (e && std::atoi(e) == 0) return false;
  if (ctx->fused_off_call || ctx->fused_disabled) return false;  // repetition of a batch whose fused launch timed out
  if (ctx->pme) return false;  // PME: generic real-space kernel + the reciprocal-space launches (pme.hip) after it
  const bool only_lj_el = c.terms != 0 && (c.terms & ~(TMDHIP_TERM_LJ | TMDHIP_TERM_ELECTROSTATICS)) == 0;
  return only_lj_el && ctx->d.ntypes <= kEntryTypes && rp.lg.lpa >= 4 && rp.lg.lpa <= 64 && kFastThreads / rp.lg.lpa <= 64;
}

// ---- a plain evaluation with energies in TWO launches behind the displacement test (tmdhip_compute, round 6) -------------------------
// Cell-list contexts in fp32 with one replica and a light topology (water, ions): the ENERGY variant of the lean pair launch with
// evaluation-only step blocks (FUSED = 5, md_step.h: FINAL = 2) that add the bonded force of their atoms to the pair force, store
// the sum in the caller's array and leave the bonded energies in the scratch rows; then ONE kernel folds the rows and reports
// energies and list flags to the caller's host-mapped zone.  The bonded kernel, its pass over the force array, the fold launch, the
// report launch and the clearing of the energy buffer go away (5 launches -> 3 with the displacement test).  Returns 1 when the
// evaluation was enqueued this way (the caller waits for ctx->obs_seq), 0 when the context does not qualify, < 0 on errors.
int compute_fused_eval(tmdhip_ctx *ctx, const void *pos_dev, const double *box, void *forces_dev, double *e_dev, double *scratch_ke,
                       double *host_e, double *host_ke, int *host_flags, volatile unsigned *host_seq, hipStream_t st) {
  const char *e_on = std::getenv("TMDHIP_FUSED_EVAL");  // (0: the separate kernels; A/B, tests)
  if (e_on && std::atoi(e_on) == 0) return 0;
  if (ctx->d.dtype != TMDHIP_F32 || ctx->algorithm != TMDHIP_ALGO_CELLLIST || ctx->rep.size() != 1 || !forces_dev || ctx->d.terms == 0 ||
      ctx->no_fused_once || ctx->pme)
    return 0;
  Replica &rp = ctx->rep[0];
  const PairConsts<float> c = make_consts<float>(ctx, box);
  if (!list_matches_box(rp, box) || !fused_step_possible<float>(ctx, rp, c)) return 0;
  BondedArgs<float> A;
  std::memset(&A, 0, sizeof(A));
  if (tmd::bonded_inline_args(ctx, box, A) != 1) return 0;
  FusedStaticT<float> now;
  std::memset(&now, 0, sizeof(now));
  now.s.n = ctx->d.natoms;
  now.s.chk.flags = rp.flags.as<int>();
  std::memcpy(&now.A, &A, sizeof(A));
  now.has_bonded = 1;
  now.nactive = ctx->nactive;
  TMD_TRY(upload_fused_static(rp, now, st));
  FusedLaunchT<float> fl{};
  fl.fst = rp.fused_dev.as<FusedStaticT<float>>();
  fl.langevin = false;
  fl.eval_only = true;
  fl.step.pos_in = (const float *)pos_dev;
  fl.step.bonded = 1;
  rp.n_compute++;
  const int rc = compute_list<float>(ctx, rp, pos_dev, box, forces_dev, e_dev,
                                     TMDHIP_WANT_FORCES | TMDHIP_WANT_ENERGY | TMDHIP_OVERWRITE_FORCES | kSpecChain, st, &fl);
  if (rc != 0) return rc < 0 ? rc : fail("tmdhip_compute: the fused evaluation could not be enqueued");
  TMD_TRY(launch_final_fold_publish(ctx, rp, e_dev, scratch_ke, host_e, host_ke, host_flags, host_seq, 0, st));
  return 1;
}

// ---- the replicas of a cell-list context in one pair + step launch (pair_fast_kernel.h: list_pair_fast_f32_batch_kernel) ----
__global__ void batch_upload_kernel(BatchRep v, BatchRep *dst) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}

// what md_run collects per replica while it walks the replicas of an iteration that ends in ONE batched launch
struct BatchItem {
  FusedLaunchT<float> fl;
  ListOnlyOut lo;
  float *pos;       // positions of this launch's forces (cur[r])
  float *home, *f;  // the caller's position / force rows of the replica
  unsigned *pub_ptr;
  unsigned pub_val;
  double box[3];
};

// One launch for the replicas of `items` (all of the context's): table entries that changed are re-uploaded (stream-ordered
// one-thread kernels), the per-launch words travel as the kernel argument.  `energy`: the call's last step (FINAL step blocks).
static int launch_replica_batch(tmdhip_ctx *ctx, std::vector<BatchItem> &items, int bonded, uint64_t noise_step, bool energy,
                                bool langevin, hipStream_t st) {
  const int nrep = (int)items.size(), n = ctx->d.natoms;
  if (ctx->pme) return fail("batched pair + step launch: not for PME contexts");
  TMD_TRY(ctx->batch_tab.ensure(sizeof(BatchRep) * (size_t)nrep));
  if ((int)ctx->batch_host.size() != nrep) {
    ctx->batch_host.assign(nrep, BatchRep{});
    for (auto &e : ctx->batch_host) std::memset(&e, 0xFF, sizeof(e));  // (matches nothing: every entry is uploaded)
  }
  const FusedGrid grid = fused_grid_shape(ctx, ctx->rep[0], bonded);
  for (int g0 = 0; g0 < nrep; g0 += kBatchMax) {
    const int gn = std::min(kBatchMax, nrep - g0);
    BatchLaunch bl;
    std::memset(&bl, 0, sizeof(bl));
    bl.nrep = gn;
    bl.pair_blocks = grid.pair_blocks;
    bl.step_blocks = grid.step_blocks;
    bl.bonded = bonded;
    bl.poll_limit = 1u << 22;  // ~4 s of polling
    bl.noise_step = noise_step;
    PairConsts<float> c0 = make_consts<float>(ctx, items[g0].box);
    for (int k = 0; k < gn; ++k) {
      const int r = g0 + k;
      Replica &rp = ctx->rep[r];
      BatchItem &it = items[r];
      TMD_TRY(begin_fused_launch(rp, n, st, bl.gen[k]));
      const PairConsts<float> c = make_consts<float>(ctx, it.box);
      BatchRep e;
      std::memset(&e, 0, sizeof(e));
      float4 *sa = rp.sorted.as<float4>(), *sb = rp.sorted_alt.as<float4>();
      e.sorted[0] = std::min(sa, sb);
      e.sorted[1] = std::max(sa, sb);
      e.pos[0] = it.home;
      e.pos[1] = rp.pos_alt.as<float>();
      e.stype = rp.stype.as<int>();
      e.order = rp.order.as<int>();
      e.nlist = rp.nlist.as<unsigned>();
      e.nneigh = rp.nneigh.as<int>();
      e.forces = it.f;
      e.escratch = ctx->escratch.as<double>() + (size_t)r * kEnergySlots * kEnergyStride;
      e.ext = rp.extent.as<int>();
      e.lflags = rp.flags.as<int>();
      e.padgen = rp.padgen.as<int>();
      e.fst = it.fl.fst;
      e.fsort = rp.fsort.as<float4>();
      e.hostpub = rp.hostpub;
      for (int x = 0; x < 3; ++x) {
        e.box[x] = c.box[x];
        e.invbox[x] = c.invbox[x];
      }
      e.maxn = rp.lg.maxn;
      if (std::memcmp(&e, &ctx->batch_host[r], sizeof(e)) != 0) {
        hipLaunchKernelGGL(batch_upload_kernel, dim3(1), dim3(64), 0, st, e, ctx->batch_tab.as<BatchRep>() + r);
        TMD_HIP(hipGetLastError());
        ctx->batch_host[r] = e;
      }
      if (it.pos != e.pos[0] && it.pos != e.pos[1]) return fail("batched pair + step launch: positions in neither buffer of the replica");
      unsigned bits = (unsigned)it.lo.lmode & kBlLmodeMask;
      if (sa == e.sorted[1]) bits |= kBlSortedCur;
      if (it.pos == e.pos[1]) bits |= kBlPosCur;
      if (it.lo.next_parity) bits |= kBlNextParity;
      if (it.fl.step.near_host) bits |= kBlReports;
      if (it.pub_ptr) bits |= kBlPublish;
      bl.bits[k] = bits;
      bl.seq[k] = it.fl.step.seq;
      bl.pub[k] = it.pub_val;
    }
    TMD_TRY(launch_pair_fast_f32_batch(ctx, g0, c0, bl, ctx->rep[g0].lg.lpa, energy, langevin, st));
  }
  return 0;
}

// ---- tmdhip_md_run ----------------------------------------------------------------------------------------------------
static bool env_is_zero(const char *name) {
  const char *e = std::getenv(name);
  return e && std::atoi(e) == 0;
}

// what an iteration knows about one replica between its pacing, its integrator kernel and its forces
template <typename R>
struct RepStep {
  int r;
  Replica &rp;
  const double *box;
  R *home, *f;  // the caller's position / force rows of the replica
  PairConsts<R> c;
  bool list;         // the forces come from the Verlet list (until a box too small for cells makes the context fall back)
  bool check;        // the displacement test rides on the integrator kernel: a list exists for this box
  bool zeroed;       // the integrator kernel clears `f` for the all-pairs launch
  bool pace = false, skip_chain = false;  // chain skipping: the host paces itself / leaves this step's rebuild chain out
  bool was_stepped = false;               // the previous pair launch has made this iteration's step
};

// One tmdhip_md_run call: the state that lives across its iterations (it = 0 .. niter: first half step of step `it` behind
// the second half of step it - 1) and the steps an iteration is made of.
template <typename R>
struct MdRun {
  using R4 = typename Vec<R>::T4;
  static constexpr bool kF32 = std::is_same<R, float>::value;
  tmdhip_ctx *const ctx;
  const tmdhip_md_desc *const d;
  const hipStream_t st;
  const int n, nrep;
  const size_t stride;
  const bool langevin;
  // The knobs, read once per call (tests switch them within a process).  TMDHIP_CHAIN_SKIP=0 switches the feature off; the two
  // DEBUG knobs let a test reach the violation + rewind path on a small box (minimum list size, "near" fraction: > 1 = an atom
  // is never reported near its limit).  TMDHIP_FUSED_FINAL=0: the separate kernels behind the last pair launch.
  // TMDHIP_BATCH_REPLICAS=0: the replica-by-replica loop; =2: the batched launch for a single replica too (A/B of the batched
  // kernel against the plain one on the same workload).  TMDHIP_REPLICA_REBUILDS=together (list_build.hip: chain_any): every
  // replica is in the batched rebuild launch as soon as one is.
  bool chain_skip_on, final_on, rebuilds_together;
  int64_t chain_min_entries;
  double chain_near;
  int batch_min;  // replicas from which an iteration batches
  MdStepArgs<R> a{};
  // where each replica's positions currently live (caller's tensor, or the context's second buffer while
  // the bonded force is evaluated inside the integrator kernel) and whether the bonded force of the
  // last evaluation is still owed to `forces`
  std::vector<R *> cur;
  std::vector<char> owed;
  std::vector<char> stepped;    // the previous pair launch of the replica has made this iteration's step (FusedStep)
  std::vector<char> finalized;  // the last pair launch made the call's final kick, bonded force and energies itself (FINAL step blocks)
  // the same for the replica-batched all-pairs mode (all replicas move together)
  R *const home_all;
  R *bcur;
  bool bowed = false;
  bool pace_timed_out = false;  // the device did not report within wait_published's limit: no more waiting in this call
  // an iteration that ends in ONE batched launch: what the walk over the replicas collects for it
  std::vector<BatchItem> batch_items;
  bool batching = false;
  int batch_bonded = 0;
  int it = 0;
  bool first = true, second = false;
  // the side terms (SideTerm, engine.h): the impulse dt / (1 - gamma dt) that stands for their acceleration in the step that
  // follows a force launch, one launch per active term in the order of the table
  bool any_side = false;
  double impulse_kick = 0;
  std::vector<const void *> impulse_pos;  // a batched iteration: where each replica's positions live, for ONE impulse launch

  MdRun(tmdhip_ctx *ctx_, const tmdhip_md_desc *d_, hipStream_t st_)
      : ctx(ctx_), d(d_), st(st_), n(ctx_->d.natoms), nrep((int)ctx_->rep.size()), stride((size_t)ctx_->d.natoms * 3),
        langevin(d_->vcoeff_dev != nullptr), cur(nrep), owed(nrep, 0), stepped(nrep, 0), finalized(nrep, 0),
        home_all((R *)d_->pos_dev), bcur((R *)d_->pos_dev) {
    for (const SideTerm &t : ctx->side) any_side = any_side || t.state;
    const char *e_min = std::getenv("TMDHIP_DEBUG_CHAIN_MIN_ENTRIES"), *e_near = std::getenv("TMDHIP_DEBUG_CHAIN_NEAR"),
               *e_batch = std::getenv("TMDHIP_BATCH_REPLICAS");
    chain_skip_on = !env_is_zero("TMDHIP_CHAIN_SKIP") && !ctx->no_chain_skip_once;
    chain_min_entries = e_min ? std::atoll(e_min) : kChainSkipMinEntries;
    chain_near = e_near ? std::atof(e_near) : kChainSkipNear;
    final_on = !env_is_zero("TMDHIP_FUSED_FINAL");
    batch_min = !e_batch ? 2 : std::atoi(e_batch) == 0 ? std::numeric_limits<int>::max() : std::atoi(e_batch) == 2 ? 1 : 2;
    rebuilds_together = read_chain_knobs().together;
    ctx->no_chain_skip_once = false;
    ctx->fused_off_call = ctx->no_fused_once;
    ctx->no_fused_once = false;
    ctx->ke_from_run = nullptr;
    ctx->run_published_seq = 0;
    a.n = n;
    a.mass = (const R *)d->mass_dev;
    a.vcoeff = (const R *)d->vcoeff_dev;
    a.dt = (R)d->dt;
    a.half_dt = (R)(0.5 * d->dt);
    a.gamma = (R)d->gamma;
    a.seed = d->seed;
    a.qs = ctx->qs.as<R>();
    for (int r = 0; r < nrep; ++r) cur[r] = (R *)d->pos_dev + r * stride;
  }

  bool list_context() const { return ctx->algorithm == TMDHIP_ALGO_CELLLIST && ctx->d.terms != 0; }
  bool wants_energy() const { return it == d->niter - 1 && d->energies_dev; }
  // THE definition of "the pair launch of this replica can make a step": a list built for this box, a lean kernel, no
  // constraints (the unfused kernels only — a step block owns 64 cell-sorted atoms, a water's atoms straddle them)
  bool can_fuse(const Replica &rp, const double *box, const PairConsts<R> &c) const {
    return list_context() && list_matches_box(rp, box) && !ctx->cons && fused_step_possible<R>(ctx, rp, c);
  }
  // ... and of the steps it can make.  Interior steps: the launch makes the next step.  The last step of a call that wants
  // energies (`en`): the launch makes the final kick, the bonded force + energies and the kinetic energy (FINAL step blocks),
  // `final_ok`: where the caller has a fold kernel behind it.
  bool fusable_step(bool en, bool final_ok) const { return en ? it + 1 == d->niter && final_ok && final_on : it + 1 < d->niter; }
  // the integrator kernel of this iteration's phase: the constrained form when the context has constraints
  void launch_step(const PairConsts<R> &c, bool check, int reps) {
    if (ctx->cons) return launch_cons_step<R>(ctx, a, c, second, langevin, first, check, reps, st);
    for_md_phase(second, langevin, first, [&](auto s, auto l, auto f) {
      launch_md_step<R, decltype(s)::value, decltype(l)::value, decltype(f)::value>(a, c, check, st, reps);
    });
  }

  int run() {
    if (any_side) TMD_TRY(check_side_terms());
    fall_back_before_the_walk();
    TMD_TRY(snapshot_unless_first_kernel_takes_it());
    for (it = 0; it <= d->niter; ++it) {
      first = it < d->niter;
      second = it > 0;
      a.noise_step = d->step0 + (uint64_t)(it > 0 ? it - 1 : 0);
      if (nrep > 1 && (ctx->algorithm == TMDHIP_ALGO_ALLPAIRS || ctx->d.terms == 0)) {
        TMD_TRY(step_all_replicas_together());
        continue;
      }
      plan_batch();
      for (int r = 0; r < nrep; ++r) {
        RepStep<R> s = begin_replica(r);
        TMD_TRY(pace(s));
        TMD_TRY(integrate(s));
        if (first) TMD_TRY(forces(s));
      }
      if constexpr (kF32) {
        if (batching) TMD_TRY(finish_batch());
      }
    }
    TMD_TRY(copy_home());
    return any_side ? finish_side_terms() : 0;
  }

  // What a run with side terms refuses: 1 - gamma dt <= 0 (in the name of the first active term), and what each term checks
  // itself (masses, boxes, state).  Sets impulse_kick = dt / (1 - gamma dt), gamma = 0 without Langevin.
  int check_side_terms() {
    const double gdt = langevin ? d->gamma * d->dt : 0.0;
    for (const SideTerm &t : ctx->side) {
      if (!t.state) continue;
      if (!(1.0 - gdt > 0.0))
        return fail(std::string("tmdhip_md_run: ") + t.needs + " 1 - gamma dt > 0 (the impulse is dt a / (1 - gamma dt))");
      TMD_TRY(t.run_check(ctx, "tmdhip_md_run", d->box_host, d->mass_dev, st));
    }
    impulse_kick = d->dt / (1.0 - gdt);
    return 0;
  }

  // vel += impulse_kick F / m of every active side term, for replicas rep0 .. rep0 + n_rep - 1 (arguments as SideTerm::launch)
  int side_impulses(int rep0, int n_rep, const void *pos, const void *const *pos_each, const double *box_host, void *vel) {
    for (const SideTerm &t : ctx->side)
      if (t.state) TMD_TRY(t.launch(ctx, rep0, n_rep, pos, pos_each, box_host, nullptr, vel, d->mass_dev, impulse_kick, nullptr, st));
    return 0;
  }

  // The side terms, the last step of the call: dt/2 a for the velocities, F for the caller's forces (total on return, and the
  // next call's first half kick is right), the term's energies.  The kinetic energy the last launch summed is stale.
  int finish_side_terms() {
    ctx->ke_from_run = nullptr;  // (before the first kick: a launch that fails leaves nothing stale published)
    ctx->run_published_seq = 0;
    for (const SideTerm &t : ctx->side)
      if (t.state)
        TMD_TRY(t.launch(ctx, 0, nrep, d->pos_dev, nullptr, d->box_host, d->forces_dev, d->vel_dev, d->mass_dev, 0.5 * d->dt, t.run_energy(ctx), st));
    return 0;
  }

  // An AUTO context falls back to all pairs, for good and for every replica, when a box is too small for cells.  With several
  // replicas that must not happen in the middle of the walk over them: a replica in front of the one with the small box has by
  // then made its next step inside its pair launch (took_step), and step_all_replicas_together, which takes over from the next
  // iteration, would make that step again.  The boxes of a call are fixed, so the same host arithmetic the re-plan runs
  // (grid_plan.h; open boundaries always get a grid, whatever the atoms' bounds) decides it here, before the first kernel.
  void fall_back_before_the_walk() {
    if (nrep < 2 || !list_context() || ctx->d.algorithm != TMDHIP_ALGO_AUTO) return;
    const double none[3] = {0, 0, 0};
    for (int r = 0; r < nrep; ++r) {
      const double *box = d->box_host + 3 * r;
      if (list_matches_box(ctx->rep[r], box)) continue;
      GridPlan p{};
      if (!plan_grid_host(n, ctx->rlist, box, none, none, read_stencil_knob(), p)) {
        ctx->algorithm = TMDHIP_ALGO_ALLPAIRS;
        return;
      }
    }
  }

  int snapshot_unless_first_kernel_takes_it() {
    if (!ctx->snap_pending) return 0;
    const size_t bytes = sizeof(R) * stride * nrep, n4 = bytes / 16;
    if (!snapshot_by_kernel(d, bytes)) {  // (buffers that the 16-byte kernels cannot read: three copies)
      const size_t padded = (bytes + 15) / 16 * 16;
      char *sn = ctx->snap.as<char>();
      TMD_HIP(hipMemcpyAsync(sn, d->pos_dev, bytes, hipMemcpyDeviceToDevice, st));
      TMD_HIP(hipMemcpyAsync(sn + padded, d->vel_dev, bytes, hipMemcpyDeviceToDevice, st));
      TMD_HIP(hipMemcpyAsync(sn + 2 * padded, d->forces_dev, bytes, hipMemcpyDeviceToDevice, st));
      ctx->snap_pending = false;
      return 0;
    }
    // the first kernel of the call takes the snapshot only when it is the plain first half step of a list replica with a valid
    // list (the common case); otherwise the copy kernel runs after all
    if (nrep == 1 && list_context() && list_matches_box(ctx->rep[0], d->box_host)) return 0;
    hipLaunchKernelGGL(snapshot3_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, n4, (const uint4 *)d->pos_dev,
                       (const uint4 *)d->vel_dev, (const uint4 *)d->forces_dev, ctx->snap.as<uint4>(), ctx->snap_zero, ctx->snap_nzero);
    TMD_HIP(hipGetLastError());
    ctx->snap_pending = false;
    return 0;
  }

  // All-pairs contexts (or none of the pair terms) with several replicas: small systems are launch-bound, one launch of every
  // kernel serves all replicas
  int step_all_replicas_together() {
    for (int r = 0; r < nrep; ++r) {  // leftovers of a cell-list context that fell back to all pairs in this call
      R *home = home_all + r * stride;
      if (owed[r]) {
        TMD_TRY(tmdhip_compute_bonded(ctx, r, cur[r], d->box_host + 3 * r, (R *)d->forces_dev + r * stride, nullptr,
                                      TMDHIP_WANT_FORCES, st));
        owed[r] = 0;
      }
      if (cur[r] != home) {
        TMD_HIP(hipMemcpyAsync(home, cur[r], sizeof(R) * stride, hipMemcpyDeviceToDevice, st));
        cur[r] = home;
      }
    }
    R *f = (R *)d->forces_dev;
    const PairConsts<R> c = make_consts<R>(ctx, d->box_host);
    a.pos_in = a.pos_out = bcur;
    a.vel = (R *)d->vel_dev;
    a.f = f;
    a.f_zero = (first && ctx->d.terms != 0) ? f : nullptr;  // saves the zero-fill launch of the all-pairs path
    a.row0 = 0;
    BondedArgs<R> A;
    if (bowed) {
      // (second && first) the bonded force of step it-1 is evaluated inside the integrator kernel from
      // the undrifted positions in bcur; the drifted ones go to the other buffer
      const bool ok = tmd::bonded_inline_args(ctx, d->box_host, A) == 1;
      const R *boxes = (const R *)tmd::set_boxes(ctx, d->box_host, st);
      if (!ok || !boxes) return fail("tmdhip_md_run: inline bonded state lost");
      R *other = bcur == home_all ? ctx->pos_alt_all.as<R>() : home_all;
      a.pos_out = other;
      launch_md_step_bonded<R>(a, c, A, langevin, false, boxes, nrep, st);
      bcur = other;
      bowed = false;
    } else {
      launch_step(c, false, nrep);
    }
    TMD_HIP(hipGetLastError());
    if (!first) return 0;
    R *pos = bcur;
    if (any_side && it + 1 < d->niter) TMD_TRY(side_impulses(0, nrep, pos, nullptr, d->box_host, d->vel_dev));
    int flags_c = TMDHIP_WANT_FORCES;
    double *en = nullptr;
    if (wants_energy()) {
      flags_c |= TMDHIP_WANT_ENERGY;
      en = d->energies_dev;
    }
    const int bmode = tmd::bonded_inline_args(ctx, d->box_host, A);  // 0 none, 1 light, 2 heavy topology
    bool bonded_done = bmode == 0;
    if (ctx->d.terms != 0) {
      for (auto &rp : ctx->rep) rp.n_compute++;
      // heavy topologies, few atoms in total (launch-bound): the bonded terms ride on the all-pairs launch
      // (one wave per atom).  Measured: alanine dipeptide x1 39 -> 32 us/step, but x16 replicas 84 -> 94.
      const bool ride = bmode == 2 && (size_t)n * nrep <= kRideMaxAtoms;
      TMD_TRY(launch_allpairs<R>(ctx, pos, d->box_host, f, en, flags_c | TMDHIP_OVERWRITE_FORCES | kForcesZeroed,
                                 nullptr, st, nrep, ride ? &A : nullptr));
      for (int r = 0; r < nrep && ctx->pme; ++r)  // reciprocal-space part of every replica (pme.hip)
        TMD_TRY(pme_hook(ctx, r, pos + r * stride, d->box_host + 3 * r, f + r * stride, en ? en + (size_t)r * TMDHIP_NENERGY : nullptr,
                         flags_c, st));
      bonded_done = bonded_done || ride;
    } else {
      TMD_HIP(hipMemsetAsync(f, 0, sizeof(R) * stride * nrep, st));
    }
    if (bonded_done) return 0;
    if (it + 1 < d->niter && bmode == 1 && !ctx->cons) {
      TMD_TRY(ctx->pos_alt_all.ensure(sizeof(R) * stride * nrep));
      bowed = true;  // the next integrator kernel evaluates this step's bonded force itself
    } else {
      TMD_TRY(tmdhip_compute_bonded(ctx, TMDHIP_ALL_REPLICAS, pos, d->box_host, f, en, flags_c, st));
    }
    return 0;
  }

  // The replicas of a cell-list context in ONE pair + step launch (round 6): when every replica of this iteration would make a
  // fused launch of its own, the walk over the replicas does the per-replica part (pacing, the first half step of a call, the
  // rebuild chain) and the launch follows behind it (finish_batch).  Beyond can_fuse: nothing owed or finalized, and one kernel
  // shape (lanes per atom, bonded mode) for all.
  void plan_batch() {
    batching = kF32 && first && nrep >= batch_min && list_context() && fusable_step(wants_energy(), true);
    batch_bonded = 0;
    for (int r = 0; batching && r < nrep; ++r) {
      const Replica &rp = ctx->rep[r];
      const double *box = d->box_host + 3 * r;
      BondedArgs<R> A;
      std::memset(&A, 0, sizeof(A));
      batching = can_fuse(rp, box, make_consts<R>(ctx, box)) && !owed[r] && !finalized[r] && rp.lg.lpa == ctx->rep[0].lg.lpa;
      if (batching) {
        const int bm = tmd::bonded_inline_args(ctx, box, A);
        batching = bm >= 0 && (r == 0 || bm == batch_bonded);
        batch_bonded = bm;
      }
    }
    if (batching) batch_items.resize(nrep);
  }

  RepStep<R> begin_replica(int r) {
    Replica &rp = ctx->rep[r];
    const double *box = d->box_host + 3 * r;
    R *f = (R *)d->forces_dev + r * stride;
    const bool list = list_context();
    a.vel = (R *)d->vel_dev + r * stride;
    a.f = f;
    a.f_zero = (first && !list && ctx->d.terms != 0) ? f : nullptr;
    a.row0 = (uint64_t)r * (uint64_t)n;
    rp.skin_vel = a.vel;  // a rebuild in this step sizes the skins from the current velocities
    a.chk = make_check<R>(ctx, rp);
    // the displacement test can ride on the integrator kernel when a list exists for this box
    return {r, rp, box, (R *)d->pos_dev + r * stride, f, make_consts<R>(ctx, box), list, first && list && list_matches_box(rp, box),
            a.f_zero != nullptr};
  }

  // Chain skipping (ListCheck): on large lists the host stays one step behind the device — it waits until the
  // pair kernel of the previous step has started (45 us of kernel time are then still ahead of it) — and
  // leaves the rebuild chain out when no atom was near its limit in that step.  On the first step of a call only
  // if the caller says that nothing has moved since the previous one (tmdhip_md_desc::continuation; the report is
  // then the previous call's last), never in the repetition of a rewound batch.
  int pace(RepStep<R> &s) {
    s.pace = s.check && chain_skip_on && (int64_t)n * s.rp.lg.maxn >= chain_min_entries;
    if (s.pace) return pace_behind_device<R>(s.rp, a.chk, it > 0 || d->continuation != 0, chain_near, pace_timed_out, s.skip_chain);
    // (the final kick of a call — it == niter, no drift, no test — leaves the report of the call's last step valid:
    // that is what the next call's first step looks at when the caller vouches for a continuation.  Round 4: this
    // branch used to clear it for every iteration without pacing, which made the hint a no-op.)
    if (first) s.rp.seq_valid = false;
    s.rp.pub_ptr = nullptr;
    return 0;
  }

  // this iteration's kicks and drift of the replica, by whoever makes them
  int integrate(RepStep<R> &s) {
    Replica &rp = s.rp;
    const int r = s.r;
    a.sorted = rp.sorted.as<R4>();
    a.inv = rp.inv.as<int>();
    a.pos_in = a.pos_out = cur[r];
    s.was_stepped = stepped[r] != 0;
    stepped[r] = 0;
    if (finalized[r]) {
      // (it == niter: the final kick was made by the step blocks of the last pair launch)
    } else if (s.was_stepped) {
      // kicks, drift, displacement test and cell-sorted records of this iteration: done by the previous pair
      // launch's epilogue (cur[r] and rp.sorted already point at its output)
    } else if (owed[r]) {
      // second && first always holds here: the bonded force of step it-1 is evaluated from the
      // undrifted positions in cur[r], the drifted ones go to the other buffer
      BondedArgs<R> A;
      std::memset(&A, 0, sizeof(A));
      if (tmd::bonded_inline_args(ctx, s.box, A) != 1) return fail("tmdhip_md_run: inline bonded state lost");
      R *other = cur[r] == s.home ? rp.pos_alt.as<R>() : s.home;
      a.pos_out = other;
      launch_md_step_bonded<R>(a, s.c, A, langevin, s.check, nullptr, 1, st);
      cur[r] = other;
      owed[r] = 0;
    } else if (first && !second) {
      // Every fused step moves the positions to the other buffer; with an odd number of them ahead (all interior
      // steps of the call, if the first one can be fused) the drift of this first step goes to the second buffer,
      // so that the call ends in the caller's tensor without a copy.  (Whatever the call's last step does: no look at `en`.)
      if (s.check && cur[r] == s.home && d->niter >= 2 && ((d->niter - 1) & 1) && can_fuse(rp, s.box, s.c)) {
        TMD_TRY(rp.pos_alt.ensure(sizeof(R) * stride));
        a.pos_out = rp.pos_alt.as<R>();
        cur[r] = a.pos_out;
      }
      if (ctx->snap_pending && s.check && nrep == 1) {  // (tmdhip_md_run left the snapshot of the entry state to this kernel)
        const size_t padded = (sizeof(R) * stride + 15) / 16 * 16;
        a.snap_pos = ctx->snap.as<R>();
        a.snap_vel = (R *)(ctx->snap.as<char>() + padded);
        a.snap_f = (R *)(ctx->snap.as<char>() + 2 * padded);
        a.zero = ctx->snap_zero;
        a.nzero = ctx->snap_nzero;
        ctx->snap_pending = false;
      }
      launch_step(s.c, s.check, 1);
      a.snap_pos = a.snap_vel = a.snap_f = nullptr;
      a.zero = nullptr;
    } else {
      launch_step(s.c, s.check, 1);
    }
    TMD_HIP(hipGetLastError());
    return 0;
  }

  // The pair launch of the replica makes a step itself (FusedStepT) where it can: `fuse`, with the launch's arguments in `fl`.
  int fused_launch_args(const RepStep<R> &s, R *pos, double *en, FusedLaunchT<R> &fl, bool &fuse) {
    Replica &rp = s.rp;
    BondedArgs<R> A;
    std::memset(&A, 0, sizeof(A));
    // (the call's last step: FINAL step blocks need the fold kernel of one replica, or of the batch)
    const int bm = (s.check && fusable_step(en != nullptr, (nrep == 1 || batching) && kF32) && can_fuse(rp, s.box, s.c))
                       ? tmd::bonded_inline_args(ctx, s.box, A) : -1;
    fuse = bm >= 0;
    if (!fuse) return 0;
    if (bm == 2) {
      // heavy topology: the bonded force depends on the positions only — it is evaluated in front of the
      // pair launch into a buffer of its own and the step blocks add it (same values, same order as the
      // separate kernels: pair force stored, bonded force added, divided by the mass)
      // (the final step: with its energies, which the bonded kernel folds into the call's buffer itself)
      TMD_TRY(rp.fbond.ensure(sizeof(R) * stride));
      TMD_TRY(tmdhip_compute_bonded(ctx, s.r, pos, s.box, rp.fbond.p, en,
                                    TMDHIP_WANT_FORCES | TMDHIP_OVERWRITE_FORCES | (en ? TMDHIP_WANT_ENERGY : 0), st));
    }
    FusedStaticT<R> now;
    fused_static_common<R>(now, n, a.vel, a.mass, a.vcoeff, d->dt, a.gamma, a.seed, a.row0, a.qs, a.inv, a.chk, chain_near);
    if (bm == 1) std::memcpy(&now.A, &A, sizeof(A));
    now.has_bonded = bm;
    now.fbond = bm == 2 ? rp.fbond.as<R>() : nullptr;
    now.nactive = 0x7fffffff;
    TMD_TRY(rp.pos_alt.ensure(sizeof(R) * stride));
    return fused_launch_common<R>(rp, now, langevin, pos, pos == s.home ? rp.pos_alt.as<R>() : s.home, d->step0 + (uint64_t)it, s.pace, fl, st);
  }

  // forces of step `it` (forces.py:122-319): nonbonded stores (list path) or accumulates into zeros
  int forces(RepStep<R> &s) {
    Replica &rp = s.rp;
    const int r = s.r;
    R *pos = cur[r];
    // (positions x_{it+1}, velocities v_{it+1/2} on every path: the step behind this launch turns the impulse into a_r's kicks)
    if (any_side && it + 1 < d->niter) {
      if (batching) {  // (one launch for all replicas in front of finish_batch's)
        impulse_pos.resize(nrep);
        impulse_pos[r] = pos;
      } else {
        TMD_TRY(side_impulses(r, 1, pos, nullptr, s.box, (R *)d->vel_dev + r * stride));
      }
    }
    int flags_c = TMDHIP_WANT_FORCES;
    double *en = nullptr;
    if (wants_energy()) {
      flags_c |= TMDHIP_WANT_ENERGY;
      en = d->energies_dev + (size_t)r * TMDHIP_NENERGY;
    }
    BondedArgs<R> A;
    std::memset(&A, 0, sizeof(A));
    if (ctx->d.terms != 0) {
      rp.n_compute++;
      if (s.list) {
        bool complete = false;
        TMD_TRY(list_forces(s, pos, flags_c, en, complete));
        if (complete) return 0;
      }
      if (!s.list) {
        // heavy topology, small system: bonded terms in the same launch
        const bool ride = tmd::bonded_inline_args(ctx, s.box, A) == 2 && (size_t)n <= kRideMaxAtoms;
        TMD_TRY(launch_allpairs<R>(ctx, pos, s.box, s.f, en, flags_c | TMDHIP_OVERWRITE_FORCES | (s.zeroed ? kForcesZeroed : 0), nullptr,
                                   st, 1, ride ? &A : nullptr));
        TMD_TRY(pme_hook(ctx, r, pos, s.box, s.f, en, flags_c, st));
        if (ride) return 0;  // forces (and energies) of this step are complete
      }
    } else {
      TMD_HIP(hipMemsetAsync(s.f, 0, sizeof(R) * stride, st));
    }
    // interior step: the next integrator kernel evaluates this step's bonded force itself
    // (md_step_bonded_kernel); `forces` holds the pair part until then.  (All-pairs contexts with several
    // replicas take step_all_replicas_together from the next iteration on.)
    if (((s.list && rp.have_list) || (!s.list && nrep == 1)) && it + 1 < d->niter && !ctx->cons &&
        tmd::bonded_inline_args(ctx, s.box, A) == 1) {
      TMD_TRY(rp.pos_alt.ensure(sizeof(R) * stride));
      owed[r] = 1;
    } else {
      TMD_TRY(tmdhip_compute_bonded(ctx, r, pos, s.box, s.f, en, flags_c, st));
    }
    return 0;
  }

  // The list launch of the replica and its outcomes.  `complete`: nothing is left to do for this step — the launch was FINAL,
  // or made the next step (its forces never reach `forces`), or the replica's blocks are in the batched launch behind the
  // walk.  Otherwise the bonded part follows, behind an all-pairs launch if the box turned out too small for cells (s.list).
  int list_forces(RepStep<R> &s, R *pos, int flags_c, double *en, bool &complete) {
    Replica &rp = s.rp;
    const int r = s.r;
    FusedLaunchT<R> fl{};
    bool fuse = false;
    TMD_TRY(fused_launch_args(s, pos, en, fl, fuse));
    const int flags_l = flags_c | TMDHIP_OVERWRITE_FORCES | (s.check ? kPrechecked : 0) | (s.skip_chain ? kSkipChain : 0) |
                        (s.skip_chain && s.was_stepped ? kViolationCheck : 0);
    complete = true;
    if constexpr (kF32) {
      if (batching) {  // list bookkeeping of this replica now, its blocks in the launch behind the walk
        if (!fuse) return fail("tmdhip_md_run: a replica of the batch cannot make a fused launch");
        BatchItem &bi = batch_items[r];
        bi.fl = fl;
        bi.pos = pos;
        bi.home = s.home;
        bi.f = s.f;
        for (int k = 0; k < 3; ++k) bi.box[k] = s.box[k];
        bi.lo = ListOnlyOut{};
        TMD_TRY(compute_list<R>(ctx, rp, pos, s.box, s.f, en, flags_l | kListOnly | kDeferChain, st, &fl, &bi.lo));
        bi.pub_ptr = rp.pub_ptr;
        bi.pub_val = rp.pub_val;
        rp.pub_ptr = nullptr;
        return 0;
      }
    }
    BondedArgs<R> A;
    const int rc = compute_list<R>(ctx, rp, pos, s.box, s.f, en,
                                   flags_l | (en && !fuse && rp.have_list && tmd::bonded_inline_args(ctx, s.box, A) != 0 ? kDeferFold : 0),
                                   st, fuse ? &fl : nullptr);
    rp.pub_ptr = nullptr;
    if (fuse && rc == 0 && en) {
      TMD_TRY(took_final(true));  // (a lone launch is FINAL only in a context of one replica: fused_launch_args)
    } else if (fuse && rc == 0) {
      took_step(r, fl.step.pos_out);
    } else if (rc == kFallbackAllPairs) {
      ctx->algorithm = TMDHIP_ALGO_ALLPAIRS;
      s.list = complete = false;
    } else if (rc != 0) {
      return rc;
    } else {
      complete = false;
      TMD_TRY(pme_hook(ctx, r, pos, s.box, s.f, en, flags_c, st));
    }
    return 0;
  }

  // The aftermath of a fused launch, lone or batched.  It made the next step of replica r: positions and cell-sorted records of
  // the coming iteration are the launch's output.
  void took_step(int r, R *pos_out) {
    cur[r] = pos_out;
    fused_step_made(ctx->rep[r]);
    stepped[r] = 1;
  }
  // It made the call's last step of every replica (FINAL step blocks): forces (pair + bonded) are in `forces`, velocities kicked;
  // one fold block per replica adds its scratch rows (pair, bonded, kinetic) into the call's energy buffer and the context's
  // kinetic-energy words (tmdhip_md_observe need not sum them) — `report`: one replica, and the same kernel reports them to the
  // host (tmdhip_md_observe then only waits for the word)
  int took_final(bool report) {
    TMD_TRY(ctx->obs_ke.ensure(sizeof(double) * ctx->rep.size()));
    if (report) {
      TMD_TRY(publish_final_step(ctx, ctx->rep[0], d->energies_dev, st));
    } else {
      hipLaunchKernelGGL(final_fold_kernel, dim3(nrep), dim3(kEnergySlots), 0, st, ctx->escratch.as<double>(), d->energies_dev,
                         ctx->obs_ke.as<double>());
      TMD_HIP(hipGetLastError());
    }
    std::fill(finalized.begin(), finalized.end(), 1);
    ctx->ke_from_run = d->vel_dev;
    ctx->ke_from_run_mass = d->mass_dev;
    ctx->final_steps_in_pair_launch++;
    return 0;
  }

  int finish_batch() {
    const bool want_e = wants_energy();
    // (all replicas in one launch per term and 16 replicas, replica r's positions at impulse_pos[r])
    if (any_side && it + 1 < d->niter) TMD_TRY(side_impulses(0, nrep, nullptr, impulse_pos.data(), d->box_host, d->vel_dev));
    {  // the rebuild chains the host has not left out: one launch per kernel for all of them
      std::vector<int> reps, par;
      std::vector<const float *> ps;
      std::vector<const double *> bx;
      bool any_chain = false;
      for (int r = 0; r < nrep; ++r) any_chain = any_chain || batch_items[r].lo.chain;
      const bool everybody = any_chain && rebuilds_together;
      for (int r = 0; r < nrep; ++r)
        if (batch_items[r].lo.chain || everybody) {
          reps.push_back(r);
          // (a replica whose chain the host had left out: compute_list has counted the step already)
          par.push_back(batch_items[r].lo.chain ? batch_items[r].lo.chain_parity : (int)((ctx->rep[r].step - 1) & 1));
          ps.push_back(batch_items[r].pos);
          bx.push_back(batch_items[r].box);
        }
      if (!reps.empty()) TMD_TRY(enqueue_chain_batch<float>(ctx, (int)reps.size(), reps.data(), ps.data(), par.data(), bx.data(), st));
    }
    TMD_TRY(launch_replica_batch(ctx, batch_items, batch_bonded, d->step0 + (uint64_t)it, want_e, langevin, st));
    if (want_e) return took_final(false);
    for (int r = 0; r < nrep; ++r) took_step(r, batch_items[r].fl.step.pos_out);
    return 0;
  }

  int copy_home() {
    if (bcur != home_all) TMD_HIP(hipMemcpyAsync(home_all, bcur, sizeof(R) * stride * nrep, hipMemcpyDeviceToDevice, st));
    for (int r = 0; r < nrep; ++r) {
      R *home = (R *)d->pos_dev + r * stride;
      if (cur[r] != home) TMD_HIP(hipMemcpyAsync(home, cur[r], sizeof(R) * stride, hipMemcpyDeviceToDevice, st));
    }
    return 0;
  }
};

template <typename R>
int md_run(tmdhip_ctx *ctx, const tmdhip_md_desc *d, hipStream_t st) {
  return MdRun<R>(ctx, d, st).run();
}

template bool fused_step_possible<float>(const tmdhip_ctx *, const Replica &, const PairConsts<float> &);
template bool fused_step_possible<double>(const tmdhip_ctx *, const Replica &, const PairConsts<double> &);
template int md_run<float>(tmdhip_ctx *, const tmdhip_md_desc *, hipStream_t);
template int md_run<double>(tmdhip_ctx *, const tmdhip_md_desc *, hipStream_t);

}  // namespace tmd

using namespace tmd;

extern "C" {

int tmdhip_md_run(tmdhip_ctx *ctx, const tmdhip_md_desc *desc, void *stream) {
  if (!ctx || !desc) return fail("tmdhip_md_run: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_md_desc)) return fail("tmdhip_md_run: tmdhip_md_desc size mismatch (ABI)");
  if (desc->niter < 0) return fail("tmdhip_md_run: niter must be >= 0");
  if (!desc->pos_dev || !desc->vel_dev || !desc->forces_dev || !desc->mass_dev || !desc->box_host)
    return fail("tmdhip_md_run: null buffer");
  if (desc->niter == 0) return 0;
  // tmdhip_md_restore answers for THIS call from here on: a call that is refused before its snapshot is enqueued (the checks
  // below, a side term's run_check) or that takes none (an all-pairs context) must not leave an earlier call's entry state on offer
  ctx->snap_bytes = 0;
  if (ctx->vsites && !cons_has_sites(ctx))
    return fail("tmdhip_md_run: a context with virtual sites steps them with their rigid waters: set the constraints "
                "(tmdhip_set_constraints after tmdhip_set_vsites)");
  hipStream_t st = (hipStream_t)stream;
  const int nzero = (int)(TMDHIP_NENERGY * ctx->rep.size());
  bool zeroed = desc->energies_dev == nullptr;
  size_t snap_wanted = 0;  // bytes of the snapshot md_run's first kernel is to take (snap_pending)
  if (ctx->algorithm == TMDHIP_ALGO_CELLLIST) {
    // state at entry, for tmdhip_md_restore (a truncated list is only detected after the batch)
    const size_t bytes = (size_t)ctx->real_size * 3 * ctx->d.natoms * ctx->rep.size();
    const size_t padded = (bytes + 15) / 16 * 16;
    TMD_TRY(ctx->snap.ensure(3 * padded));
    // md_run takes the snapshot once it has accepted the call (snapshot_unless_first_kernel_takes_it): its first kernel saves
    // the state itself where it can — one launch less per call —, else snapshot3_kernel, or three copies where the buffers
    // are not 16-byte aligned
    const bool fits = snapshot_by_kernel(desc, bytes) && (size_t)nzero <= bytes / 16;
    ctx->snap_pending = true;
    ctx->snap_zero = fits ? desc->energies_dev : nullptr;
    ctx->snap_nzero = nzero;
    zeroed = zeroed || fits;
    snap_wanted = bytes;
  }
  if (!zeroed) TMD_HIP(hipMemsetAsync(desc->energies_dev, 0, sizeof(double) * nzero, st));
  for (auto &rp : ctx->rep) rp.spec_valid = false;  // (a plain evaluation's report says nothing about positions this call moves)
  const int rc = ctx->d.dtype == TMDHIP_F32 ? md_run<float>(ctx, desc, st) : md_run<double>(ctx, desc, st);
  for (auto &rp : ctx->rep) rp.skin_vel = nullptr;  // rebuilds outside an MD run know no velocities: static skins
  // a kernel of md_run has taken the snapshot (it clears snap_pending where it enqueues it): only then is there a saved state.
  // A run that failed before that point leaves snap_bytes = 0, and tmdhip_md_restore refuses.
  if (snap_wanted && !ctx->snap_pending) ctx->snap_bytes = snap_wanted;
  if (rc == 0 && ctx->vsites) {
    // the forces of the last step leave the call spread (zero site rows), as a plain evaluation leaves them; the final kick has
    // folded the same shares in registers
    const VsiteState *V = (const VsiteState *)ctx->vsites;
    TMD_TRY(tmdhip_vsite_spread(ctx->d.dtype, (int64_t)ctx->rep.size(), ctx->d.natoms, desc->forces_dev, V->nsites, V->site.as<int32_t>(),
                                V->parent.as<int32_t>(), V->weight.as<double>(), stream));
  }
  if (rc == 0 && ctx->snap_pending) {
    ctx->snap_pending = false;
    return fail("tmdhip_md_run: the state at entry was not saved (internal error)");
  }
  ctx->snap_pending = false;
  if (rc == 0) TMD_TRY(enqueue_run_report(ctx, desc, st));
  return rc;
}

int tmdhip_md_restore(tmdhip_ctx *ctx, const tmdhip_md_desc *desc, void *stream) {
  if (!ctx || !desc) return fail("tmdhip_md_restore: null argument");
  if (!desc->pos_dev || !desc->vel_dev || !desc->forces_dev) return fail("tmdhip_md_restore: null buffer");
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = (size_t)ctx->real_size * 3 * ctx->d.natoms * ctx->rep.size();
  if (ctx->snap_bytes != bytes || !ctx->snap.p) return fail("tmdhip_md_restore: no saved state of a matching tmdhip_md_run");
  const char *sn = ctx->snap.as<char>();
  const size_t padded = (bytes + 15) / 16 * 16;
  TMD_HIP(hipMemcpyAsync(desc->pos_dev, sn, bytes, hipMemcpyDeviceToDevice, st));
  TMD_HIP(hipMemcpyAsync(desc->vel_dev, sn + padded, bytes, hipMemcpyDeviceToDevice, st));
  TMD_HIP(hipMemcpyAsync(desc->forces_dev, sn + 2 * padded, bytes, hipMemcpyDeviceToDevice, st));
  for (auto &rp : ctx->rep) rp.box[0] = -1;  // re-plan + rebuild from the restored positions
  ctx->no_chain_skip_once = true;            // and no chain is left out while the batch is repeated
  ctx->ke_from_run = nullptr;                // (the velocities are no longer those of the run that ended)
  return 0;
}

}  // extern "C"
