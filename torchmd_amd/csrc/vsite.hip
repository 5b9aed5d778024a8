// Virtual interaction sites for gfx950: place massless linear sites, hand their forces to their parents.
//
// A linear site sits at r_s = sum_k w_k r_parent_k (two or three parents, sum_k w_k = 1): the charge site of four-site water
// (TIP4P-Ew, TIP4P/2005, OPC).  tmdhip_vsite_construct writes the site rows of a position array from the parent rows;
// tmdhip_vsite_spread adds w_k F_s to every parent's force row and stores zero in the site's row — exact for a linear site
// (total force and torque are unchanged).  Molecules must be whole (no minimum image), the precondition tmdhip_scale_groups
// states.
//
// One thread per site, blockIdx.y = replica.  No two sites share a parent and no site is a parent (tmdhip_set_vsites and the
// host class check that), so every row is written by one thread: no atomics, and two calls on the same input give the same
// bits.  Arithmetic in double in both precisions, rounded once on the store, parents in table order (vsite_math.h — the
// constrained MD step uses the same two expressions for the site of a rigid water).  A row index outside [0, natoms) makes
// the thread skip its site: a bad table cannot write out of bounds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "engine.h"
#include "vsite_math.h"

using namespace tmd;

namespace {

template <typename R>
__global__ void vsite_construct_kernel(int natoms, int nsites, R *__restrict__ pos, const int *__restrict__ site,
                                       const int *__restrict__ parent, const double *__restrict__ weight) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsites) return;
  const int i = site[s], p0 = parent[3 * s], p1 = parent[3 * s + 1], p2 = parent[3 * s + 2];
  const bool three = p2 >= 0;
  if ((unsigned)i >= (unsigned)natoms || (unsigned)p0 >= (unsigned)natoms || (unsigned)p1 >= (unsigned)natoms ||
      (three && p2 >= natoms))
    return;
  R *p = pos + (size_t)blockIdx.y * (size_t)natoms * 3;
  const double w0 = weight[3 * s], w1 = weight[3 * s + 1], w2 = weight[3 * s + 2];
#pragma unroll
  for (int q = 0; q < 3; ++q)
    p[3 * i + q] = vsite_coord<R>(w0, w1, w2, p[3 * p0 + q], p[3 * p1 + q], three ? p[3 * p2 + q] : R(0), three);
}

template <typename R>
__global__ void vsite_spread_kernel(int natoms, int nsites, R *__restrict__ forces, const int *__restrict__ site,
                                    const int *__restrict__ parent, const double *__restrict__ weight) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nsites) return;
  const int i = site[s];
  if ((unsigned)i >= (unsigned)natoms) return;
  R *f = forces + (size_t)blockIdx.y * (size_t)natoms * 3;
  const R fs[3] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = parent[3 * s + k];
    if ((unsigned)a >= (unsigned)natoms) continue;  // (-1: a two-parent site)
    const double w = weight[3 * s + k];
#pragma unroll
    for (int q = 0; q < 3; ++q) f[3 * a + q] = vsite_share<R>(f[3 * a + q], w, fs[q]);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) f[3 * i + q] = R(0);
}

int check_args(const char *who, int dtype, int64_t nreplicas, int64_t natoms, const void *buf, int32_t nsites, const void *site,
               const void *parent, const void *weight) {
  if (dtype != TMDHIP_F32 && dtype != TMDHIP_F64) return fail(std::string(who) + ": bad dtype");
  if (nreplicas <= 0 || natoms <= 0 || nreplicas > 65535 || natoms > INT32_MAX / 4)
    return fail(std::string(who) + ": nreplicas must lie in 1 .. 65535 and natoms must be positive (and fit 32-bit indices)");
  if (nsites < 0 || nsites > natoms) return fail(std::string(who) + ": bad site count");
  if (!buf || (nsites && (!site || !parent || !weight))) return fail(std::string(who) + ": null pointer");
  return 0;
}

}  // namespace

namespace tmd {

void vsite_release(tmdhip_ctx *ctx) {
  VsiteState *S = (VsiteState *)ctx->vsites;
  if (!S) return;
  for (DevBuf *b : {&S->site, &S->parent, &S->weight}) b->release();
  delete S;
  ctx->vsites = nullptr;
}

}  // namespace tmd

extern "C" {

int tmdhip_vsite_construct(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, int32_t nsites, const int32_t *site_dev,
                           const int32_t *parent_dev, const double *weight_dev, void *stream) {
  TMD_TRY(check_args("tmdhip_vsite_construct", dtype, nreplicas, natoms, pos_dev, nsites, site_dev, parent_dev, weight_dev));
  if (nsites == 0) return 0;
  const dim3 grid((unsigned)((nsites + 255) / 256), (unsigned)nreplicas), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TMDHIP_F32)
    hipLaunchKernelGGL(vsite_construct_kernel<float>, grid, block, 0, st, (int)natoms, nsites, (float *)pos_dev, site_dev, parent_dev, weight_dev);
  else
    hipLaunchKernelGGL(vsite_construct_kernel<double>, grid, block, 0, st, (int)natoms, nsites, (double *)pos_dev, site_dev, parent_dev, weight_dev);
  TMD_HIP(hipGetLastError());
  return 0;
}

int tmdhip_vsite_spread(int dtype, int64_t nreplicas, int64_t natoms, void *forces_dev, int32_t nsites, const int32_t *site_dev,
                        const int32_t *parent_dev, const double *weight_dev, void *stream) {
  TMD_TRY(check_args("tmdhip_vsite_spread", dtype, nreplicas, natoms, forces_dev, nsites, site_dev, parent_dev, weight_dev));
  if (nsites == 0) return 0;
  const dim3 grid((unsigned)((nsites + 255) / 256), (unsigned)nreplicas), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TMDHIP_F32)
    hipLaunchKernelGGL(vsite_spread_kernel<float>, grid, block, 0, st, (int)natoms, nsites, (float *)forces_dev, site_dev, parent_dev, weight_dev);
  else
    hipLaunchKernelGGL(vsite_spread_kernel<double>, grid, block, 0, st, (int)natoms, nsites, (double *)forces_dev, site_dev, parent_dev, weight_dev);
  TMD_HIP(hipGetLastError());
  return 0;
}

int tmdhip_set_vsites(tmdhip_ctx *ctx, const tmdhip_vsite_desc *desc) {
  if (!ctx || !desc) return fail("tmdhip_set_vsites: null argument");
  if (desc->struct_size != (int32_t)sizeof(tmdhip_vsite_desc)) return fail("tmdhip_set_vsites: tmdhip_vsite_desc size mismatch (ABI)");
  if (ctx->cons) return fail("tmdhip_set_vsites: release the constraints first (tmdhip_set_constraints reads the site tables when it forms its units)");
  vsite_release(ctx);
  if (!desc->enable || desc->nsites <= 0) return 0;
  const int n = ctx->d.natoms, ns = desc->nsites;
  if (ns > n || !desc->site_host || !desc->parent_host || !desc->weight_host) return fail("tmdhip_set_vsites: null array or bad site count");
  std::vector<char> role(n, 0);  // 1 = site, 2 = parent
  for (int s = 0; s < ns; ++s) {
    const int i = desc->site_host[s];
    if (i < 0 || i >= n) return fail("tmdhip_set_vsites: site index out of range");
    if (role[i]) return fail("tmdhip_set_vsites: a site is listed twice");
    role[i] = 1;
  }
  for (int s = 0; s < ns; ++s) {
    double sum = 0;
    for (int k = 0; k < 3; ++k) {
      const int a = desc->parent_host[3 * s + k];
      const double w = desc->weight_host[3 * s + k];
      if (a == -1 && k == 2) continue;
      if (a < 0 || a >= n) return fail("tmdhip_set_vsites: parent index out of range");
      if (role[a] == 1) return fail("tmdhip_set_vsites: a site cannot be a parent");
      if (role[a] == 2) return fail("tmdhip_set_vsites: two sites share a parent (or a site lists one twice)");
      role[a] = 2;
      if (!(w == w) || w > 1e6 || w < -1e6) return fail("tmdhip_set_vsites: weights must be finite");
      sum += w;
    }
    if (!(sum > 1.0 - 1e-9 && sum < 1.0 + 1e-9)) return fail("tmdhip_set_vsites: the weights of a site must sum to 1");
  }
  auto *S = new VsiteState();
  ctx->vsites = S;
  S->nsites = ns;
  S->site_h.assign(desc->site_host, desc->site_host + ns);
  S->parent_h.assign(desc->parent_host, desc->parent_host + 3 * (size_t)ns);
  S->weight_h.assign(desc->weight_host, desc->weight_host + 3 * (size_t)ns);
  auto up = [&](DevBuf &b, const void *src, size_t bytes) {
    TMD_TRY(b.ensure(std::max<size_t>(bytes, 16)));
    TMD_HIP(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  int rc = up(S->site, S->site_h.data(), sizeof(int32_t) * ns);
  if (!rc) rc = up(S->parent, S->parent_h.data(), sizeof(int32_t) * 3 * ns);
  if (!rc) rc = up(S->weight, S->weight_h.data(), sizeof(double) * 3 * ns);
  if (rc) vsite_release(ctx);
  return rc;
}

}  // extern "C"
