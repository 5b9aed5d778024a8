// Launcher of the lean fp32 list pair kernel (pair_fast_kernel.h), one replica per launch.
#include "pair_fast_kernel.h"

namespace tmd {

// host side: one launch of the lean fp32 kernel over the replica's list (fl: with step blocks behind the pair blocks)
template <bool ENERGY>
int launch_pair_fast_f32(tmdhip_ctx *ctx, Replica &rp, const PairConsts<float> &c, float *f, int overwrite, hipStream_t st,
                         hipEvent_t e0, hipEvent_t e1, int lmode, const FusedLaunch *fl) {
  const int n = ctx->d.natoms;
  const bool lj = c.terms & TMDHIP_TERM_LJ, el = c.terms & TMDHIP_TERM_ELECTROSTATICS;
  // (Q: charge products from the class table, pair_fast_kernel.h: QTAB)
  const bool qtab = TMD_CHARGE_TABLE && ctx->charge_by_class;
  FusedStep fstep{};
  if (fl) fstep = fl->step;
  const FusedGrid grid = fused_grid_shape(ctx, rp, fstep.bonded);
  if (fl) {
    // step blocks behind the pair blocks (interior steps of tmdhip_md_run; fused_step_possible() has been asked)
    fstep.nstep_blocks = grid.step_blocks;
    TMD_TRY(begin_fused_launch(rp, n, st, fstep.gen));
    fstep.watch_gen = fstep.gen;
    fstep.poll_limit = 1u << 22;  // ~4 s of polling
    // test knob: the step blocks of this replica's k-th fused launch wait for a launch number nobody writes
    if (const char *e = std::getenv("TMDHIP_DEBUG_STEP_TIMEOUT"))
      if (rp.fused_launches == std::atoll(e)) fstep.watch_gen ^= 0x80000000u, fstep.poll_limit = 1u << 8;
    fstep.fsort = rp.fsort.as<float4>();
  }
  // the variant with `lpa` lanes per atom and step blocks of mode `fused` (0: none) for the launch's terms
  auto launch = [&](auto lpa, auto fused) {
    dispatch_pair_terms(lj, el, c.switch_on, qtab, [&](auto a, auto b, auto s, auto q) {
      constexpr int F = decltype(fused)::value;
      launch_with_events(list_pair_fast_f32_kernel<decltype(lpa)::value, decltype(a)::value, decltype(b)::value, ENERGY, decltype(s)::value, F,
                                                   decltype(q)::value>,
                         dim3(grid.pair_blocks + (F ? fstep.nstep_blocks : 0)), dim3(kFastThreads), 0u, st, e0, e1, n, rp.sorted.as<float4>(),
                         rp.stype.as<int>(), rp.order.as<int>(), ctx->d.ntypes, ctx->tab.as<float2>(), rp.nlist.as<unsigned>(),
                         rp.nneigh.as<int>(), rp.lg.maxn, c, f, overwrite, ctx->escratch.as<double>(), rp.pub_ptr, rp.pub_val,
                         rp.extent.as<int>(), rp.flags.as<int>(), lmode, F ? fl->fst : nullptr, fstep, rp.padgen.as<int>(),
                         ctx->qclass.as<float>());
    });
  };
  if (fl) {
    const bool built = dispatch_fast_lpa(rp.lg.lpa, [&](auto lpa) {
      dispatch_fused_mode<ENERGY>(fl->langevin, fl->eval_only, [&](auto fused) { launch(lpa, fused); });
    });
    if (!built) return fail("fused MD step: unsupported lanes-per-atom");
  } else {
    const auto plain = [&](auto lpa) { launch(lpa, std::integral_constant<int, 0>{}); };
    if (!dispatch_fast_lpa(rp.lg.lpa, plain)) plain(std::integral_constant<int, 8>{});  // (pick_lpa never returns less than 4)
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

template int launch_pair_fast_f32<true>(tmdhip_ctx *, Replica &, const PairConsts<float> &, float *, int, hipStream_t,
                                        hipEvent_t, hipEvent_t, int, const FusedLaunch *);
template int launch_pair_fast_f32<false>(tmdhip_ctx *, Replica &, const PairConsts<float> &, float *, int, hipStream_t,
                                         hipEvent_t, hipEvent_t, int, const FusedLaunch *);

}  // namespace tmd

#ifdef TMD_PAIR_TIMELINE
extern "C" int tmdhip_debug_pair_timeline(void *out, size_t bytes) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(tmd::g_pair_timeline), std::min(bytes, sizeof(tmd::g_pair_timeline))) == hipSuccess ? 0 : -1;
}
#endif
