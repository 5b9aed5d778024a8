// Launcher of the replica-batched form of the lean fp32 list pair kernel (pair_fast_kernel.h: list_pair_fast_f32_batch_kernel):
// the pair blocks and the step blocks of up to kBatchMax replicas of a cell-list context in ONE launch.  A translation unit of
// its own so that its kernel variants compile beside those of pair_fast_f32.hip, not behind them.
//
// Reference semantics: the replica loop of torchmd/forces.py:105,116 over torchmd/systems.py:6-18's [R, N, 3] tensors.
#include "pair_fast_kernel.h"

namespace tmd {

int launch_pair_fast_f32_batch(tmdhip_ctx *ctx, int rep0, const PairConsts<float> &c, const BatchLaunch &bl, int lpa, bool energy,
                               bool langevin, hipStream_t st) {
  const bool lj = c.terms & TMDHIP_TERM_LJ, el = c.terms & TMDHIP_TERM_ELECTROSTATICS;
  const dim3 grid((unsigned)bl.nrep * (unsigned)(bl.pair_blocks + bl.step_blocks)), block(kFastThreads);
  const BatchRep *reps = ctx->batch_tab.as<BatchRep>() + rep0;
  // (Q: charge products from the class table, pair_fast_kernel.h: QTAB)
  const bool qtab = TMD_CHARGE_TABLE && ctx->charge_by_class;
  // the variants with L lanes per atom and energies or not (E: the call's last step) for the launch's step mode and terms
  auto launch = [&](auto L, auto E) {
    dispatch_fused_mode<decltype(E)::value>(langevin, false, [&](auto F) {
      if constexpr (decltype(F)::value != 5)  // (every batched launch makes a step: no evaluation-only variant of this kernel)
        dispatch_pair_terms(lj, el, c.switch_on, qtab, [&](auto A, auto B, auto S, auto Q) {
          hipLaunchKernelGGL((list_pair_fast_f32_batch_kernel<decltype(L)::value, decltype(A)::value, decltype(B)::value, decltype(E)::value,
                                                              decltype(S)::value, decltype(F)::value, decltype(Q)::value>),
                             grid, block, 0, st, ctx->d.natoms, ctx->d.ntypes, ctx->tab.as<float2>(), c, reps, bl, ctx->qclass.as<float>());
        });
    });
  };
  const bool built = dispatch_fast_lpa(lpa, [&](auto L) {
    if (energy) launch(L, std::true_type{});
    else launch(L, std::false_type{});
  });
  if (!built) return fail("batched pair + step launch: unsupported lanes-per-atom");
  TMD_HIP(hipGetLastError());
  ctx->batched_launches++;
  return 0;
}

}  // namespace tmd
