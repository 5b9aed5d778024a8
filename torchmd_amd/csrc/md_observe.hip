// The observables of the nonbonded engine for gfx950 (MI355X): the kernels that report energies, kinetic energies and list flags
// to host-mapped memory behind a sequence word, the report an MD run enqueues behind its last kernel, and tmdhip_md_observe.
#include "engine.h"

namespace tmd {

// tmdhip_md_observe: the per-term energies, the kinetic energies and the list flags of every replica written
// straight into host-mapped memory by one small block, followed by a sequence word the host spins on — instead of
// three device-to-host copy commands and a stream synchronisation (whose wake-up is the slowest part of a short
// call).  flags.p[r] = replica r's int[F_COUNT], or null.
struct ObsFlagPtrs {
  const int *p[16];
};
__global__ void observe_publish_kernel(int nrep, const double *__restrict__ energies, const double *__restrict__ ke,
                                       ObsFlagPtrs flags, double *host_e, double *host_ke, int *host_flags,
                                       unsigned *host_seq, unsigned seq) {
  const int t = threadIdx.x;
  for (int k = t; k < nrep * TMDHIP_NENERGY; k += blockDim.x) host_e[k] = energies ? energies[k] : 0.0;
  for (int k = t; k < nrep; k += blockDim.x) host_ke[k] = ke ? ke[k] : 0.0;
  for (int k = t; k < nrep * F_COUNT; k += blockDim.x) {
    const int r = k / F_COUNT;
    host_flags[k] = flags.p[r] ? flags.p[r][k - r * F_COUNT] : 0;
  }
  __threadfence_system();
  __syncthreads();
  if (t == 0) __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// host side of observe_publish_kernel: spin until the device has written `seq` (all results are then in place)
int wait_observed(volatile unsigned *hseq, unsigned seq, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 1; *hseq != seq; ++spins) {
    __builtin_ia32_pause();
    if ((spins & 0xFFFFu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
      TMD_HIP(hipStreamSynchronize(st));  // surfaces a device error if there is one
      if (*hseq != seq) return fail("the device did not report the results of the call");
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

// the launch of the report alone (<= 16 replicas); the caller waits for ctx->obs_seq (wait_observed) when it needs the values
static int launch_publish(tmdhip_ctx *ctx, const double *energies_dev, const double *ke_dev, bool lists, double *host_e,
                          double *host_ke, int *host_flags, volatile unsigned *host_seq, hipStream_t st) {
  const size_t nrep = ctx->rep.size();
  ObsFlagPtrs fp{};
  for (size_t r = 0; r < nrep; ++r) fp.p[r] = lists ? ctx->rep[r].flags.as<int>() : nullptr;
  ctx->obs_seq = next_seq(ctx->obs_seq);
  hipLaunchKernelGGL(observe_publish_kernel, dim3(1), dim3(128), 0, st, (int)nrep, energies_dev, ke_dev, fp, host_e, host_ke,
                     host_flags, const_cast<unsigned *>(host_seq), ctx->obs_seq);
  TMD_HIP(hipGetLastError());
  return 0;
}

int publish_observables(tmdhip_ctx *ctx, const double *energies_dev, const double *ke_dev, bool lists, double *host_e,
                        double *host_ke, int *host_flags, volatile unsigned *host_seq, hipStream_t st) {
  TMD_TRY(launch_publish(ctx, energies_dev, ke_dev, lists, host_e, host_ke, host_flags, host_seq, st));
  return wait_observed(host_seq, ctx->obs_seq, st);
}

// the host-mapped landing zone of tmdhip_md_observe: energies [R][NENERGY] | kinetic energies [R] | list flags [R][F_COUNT] | sequence word
struct ObsHost {
  double *e, *ke;
  int *flags;
  volatile unsigned *seq;
};
static int obs_host_zone(tmdhip_ctx *ctx, ObsHost &z) {
  const size_t nrep = ctx->rep.size();
  const size_t ebytes = sizeof(double) * TMDHIP_NENERGY * nrep, kbytes = sizeof(double) * nrep, fbytes = sizeof(int) * F_COUNT * nrep;
  if (!ctx->obs_host) {
    TMD_HIP(hipHostMalloc(&ctx->obs_host, ebytes + kbytes + fbytes + 64, hipHostMallocMapped));
    std::memset(ctx->obs_host, 0, ebytes + kbytes + fbytes + 64);
  }
  z.e = (double *)ctx->obs_host;
  z.ke = z.e + TMDHIP_NENERGY * nrep;
  z.flags = (int *)((char *)ctx->obs_host + ebytes + kbytes);
  z.seq = (volatile unsigned *)((char *)ctx->obs_host + ebytes + kbytes + fbytes + 32);
  return 0;
}

// The last kernel of a tmdhip_md_run call whose final step was made by FINAL step blocks (one replica): final_fold_kernel's sums
// AND observe_publish_kernel's report in one launch (round 6) — the energies of the call, the kinetic energy and the list flags go
// to the host-mapped zone with the sequence word behind them, so that a tmdhip_md_observe(TMDHIP_OBSERVE_AFTER_RUN) launches
// nothing and only waits for the word.
__global__ __launch_bounds__(kEnergySlots) void final_fold_publish_kernel(double *__restrict__ scratch, double *__restrict__ out,
                                                                          double *__restrict__ ke, const int *__restrict__ flags,
                                                                          double *host_e, double *host_ke, int *host_flags,
                                                                          unsigned *host_seq, unsigned seq, int accumulate) {
  __shared__ double part[kEnergySlots / 64][TMDHIP_NENERGY + 1];
  double *row = scratch + (size_t)threadIdx.x * kEnergyStride;
#pragma unroll
  for (int k = 0; k <= TMDHIP_NENERGY; ++k) {
    const double v = row[k];
    if (v != 0.0) row[k] = 0.0;
    const double s = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x <= TMDHIP_NENERGY) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kEnergySlots / 64; ++w) s += part[w][threadIdx.x];
    if (threadIdx.x < TMDHIP_NENERGY) {
      // (accumulate: the bonded kernel of a heavy topology has left its energies there already; a plain evaluation overwrites)
      const double e = accumulate ? out[threadIdx.x] + s : s;
      if (s != 0.0 || !accumulate) out[threadIdx.x] = e;
      host_e[threadIdx.x] = e;
    } else {
      ke[0] = s;
      host_ke[0] = s;
    }
  } else if (threadIdx.x >= 64 && threadIdx.x < 64 + F_COUNT) {
    host_flags[threadIdx.x - 64] = flags ? flags[threadIdx.x - 64] : 0;
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// final_fold_publish_kernel behind a pair launch with FINAL (or evaluation-only) step blocks; the caller waits for ctx->obs_seq
int launch_final_fold_publish(tmdhip_ctx *ctx, const Replica &rp, double *out, double *ke, double *host_e, double *host_ke,
                              int *host_flags, volatile unsigned *host_seq, int accumulate, hipStream_t st) {
  ctx->obs_seq = next_seq(ctx->obs_seq);
  hipLaunchKernelGGL(final_fold_publish_kernel, dim3(1), dim3(kEnergySlots), 0, st, ctx->escratch.as<double>(), out, ke,
                     rp.flags.as<int>(), host_e, host_ke, host_flags, const_cast<unsigned *>(host_seq), ctx->obs_seq, accumulate);
  TMD_HIP(hipGetLastError());
  return 0;
}

// ... of the last step of a tmdhip_md_run call (one replica), into the zone tmdhip_md_observe reads: that call then only waits
int publish_final_step(tmdhip_ctx *ctx, const Replica &rp, double *en, hipStream_t st) {
  ObsHost z;
  TMD_TRY(obs_host_zone(ctx, z));
  TMD_TRY(launch_final_fold_publish(ctx, rp, en, ctx->obs_ke.as<double>(), z.e, z.ke, z.flags, z.seq, 1, st));
  ctx->run_published_seq = ctx->obs_seq;
  ctx->run_published_energies = en;
  return 0;
}

// A call that returns energies is followed by tmdhip_md_observe (what Integrator.step does).  Its two launches — kinetic energy,
// report to the host — are enqueued HERE, behind the run's last kernel with no host round trip between them (small systems: the
// device idled ~20 us per call between the two C calls); tmdhip_md_observe(TMDHIP_OBSERVE_AFTER_RUN) then only waits for the
// sequence word.  (One replica on the lean fp32 kernel: the FINAL launch's fold kernel has reported already.)
int enqueue_run_report(tmdhip_ctx *ctx, const tmdhip_md_desc *desc, hipStream_t st) {
  const char *e_rep = std::getenv("TMDHIP_RUN_REPORTS");  // (0: tmdhip_md_observe launches them itself; A/B)
  if (!desc->energies_dev || ctx->run_published_seq != 0 || ctx->rep.size() > 16 || (e_rep && std::atoi(e_rep) == 0)) return 0;
  ObsHost z;
  TMD_TRY(obs_host_zone(ctx, z));
  TMD_TRY(ctx->obs_ke.ensure(sizeof(double) * ctx->rep.size()));
  if (ctx->ke_from_run != desc->vel_dev || ctx->ke_from_run_mass != desc->mass_dev) {
    TMD_TRY(tmdhip_kinetic_energy(ctx->d.dtype, (int64_t)ctx->rep.size(), ctx->d.natoms, desc->vel_dev, desc->mass_dev,
                                  ctx->obs_ke.as<double>(), st));
    ctx->ke_from_run = desc->vel_dev;
    ctx->ke_from_run_mass = desc->mass_dev;
  }
  TMD_TRY(launch_publish(ctx, desc->energies_dev, ctx->obs_ke.as<double>(), ctx->algorithm == TMDHIP_ALGO_CELLLIST, z.e, z.ke, z.flags,
                         z.seq, st));
  ctx->run_published_seq = ctx->obs_seq;
  ctx->run_published_energies = desc->energies_dev;
  return 0;
}

}  // namespace tmd

using namespace tmd;

extern "C" {

int tmdhip_md_observe(tmdhip_ctx *ctx, const void *vel_dev, const void *mass_dev, const double *energies_dev,
                      double *out_host, int flags, void *stream) {
  if (!ctx || !vel_dev || !mass_dev || !out_host) return fail("tmdhip_md_observe: null argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t nrep = ctx->rep.size();
  const size_t ebytes = sizeof(double) * TMDHIP_NENERGY * nrep, kbytes = sizeof(double) * nrep;
  TMD_TRY(ctx->obs_ke.ensure(kbytes));
  ObsHost z;
  TMD_TRY(obs_host_zone(ctx, z));
  double *he = z.e, *hk = z.ke;
  int *hf = z.flags;
  volatile unsigned *hseq = z.seq;
  const bool after_run = (flags & TMDHIP_OBSERVE_AFTER_RUN) && ctx->ke_from_run == vel_dev && ctx->ke_from_run_mass == mass_dev;
  const bool published = after_run && ctx->run_published_seq != 0 && ctx->run_published_energies == energies_dev;
  const unsigned published_seq = ctx->run_published_seq;
  ctx->run_published_seq = 0;
  if (after_run) {
    // (the FINAL step blocks of the run that just ended have summed the kinetic energy of these velocities — every replica's —
    // and the caller vouches that nothing has written them since)
  } else {
    TMD_TRY(tmdhip_kinetic_energy(ctx->d.dtype, (int64_t)nrep, ctx->d.natoms, vel_dev, mass_dev, ctx->obs_ke.as<double>(), stream));
  }
  ctx->ke_from_run = nullptr;
  const bool lists = ctx->algorithm == TMDHIP_ALGO_CELLLIST;
  if (published) {  // the run's last kernel has reported already: nothing to launch
    TMD_TRY(wait_observed(hseq, published_seq, st));
  } else if (nrep <= 16) {
    TMD_TRY(publish_observables(ctx, energies_dev, ctx->obs_ke.as<double>(), lists, he, hk, hf, hseq, st));
  } else {
    if (energies_dev) TMD_HIP(hipMemcpyAsync(he, energies_dev, ebytes, hipMemcpyDeviceToHost, st));
    else std::memset(he, 0, ebytes);
    TMD_HIP(hipMemcpyAsync(hk, ctx->obs_ke.p, kbytes, hipMemcpyDeviceToHost, st));
    if (lists)
      for (size_t r = 0; r < nrep; ++r)
        TMD_HIP(hipMemcpyAsync(hf + r * F_COUNT, ctx->rep[r].flags.p, sizeof(int) * F_COUNT, hipMemcpyDeviceToHost, st));
    TMD_HIP(hipStreamSynchronize(st));
  }
  TMD_TRY(cons_verdict(ctx));  // (every kernel of the run has finished: its report has arrived)
  int verdict = 0;
  if (lists && ctx->algorithm == TMDHIP_ALGO_CELLLIST)
    for (size_t r = 0; r < nrep; ++r)
      if (ctx->rep[r].have_list) {
        const int rc = judge_flags(ctx, ctx->rep[r], hf + r * F_COUNT, st);
        if (rc < 0) return rc;
        verdict |= rc;
      }
  for (size_t r = 0; r < nrep; ++r) {
    for (int k = 0; k < TMDHIP_NENERGY; ++k) out_host[r * (TMDHIP_NENERGY + 1) + k] = energies_dev ? he[r * TMDHIP_NENERGY + k] : 0.0;
    out_host[r * (TMDHIP_NENERGY + 1) + TMDHIP_NENERGY] = hk[r];
  }
  return verdict;
}

}  // extern "C"
