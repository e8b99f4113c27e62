// C-ABI entry points of Conv2d (encoder blocks, models/vanilla_vae.py:28-29 run at :84).
#include "vae_launch.hpp"
#include "vae_wgrad.hpp"
#include "vae_c3.hpp"

using namespace vae;

// dx[n,h,w,c] = Σ_{r,s,k: h = p*S-P+r} dy'[n,p,q,k] · W[k][r][s][c]  (transposed conv of dy);
// epilogue: [+ residual gradient], g = dx·act'(z) of x's BatchNorm/LeakyReLU, Σg -> dβ, Σg·x̂ -> dγ
extern "C" int vae_conv2d_bwd_data(const vae_conv_args* a, void* stream) {
  const char* what = "conv2d_bwd_data";
  if (int rc = check_geom(a, what)) return rc;
  if (!a->dy || !a->wt || !a->dx) return fail(VAE_E_BADARG, "conv2d_bwd_data: null tensor");
  if (!xf_ok(a->dy_xf, "conv2d_bwd_data.dy") || !epi_ok(a->dx_epi, "conv2d_bwd_data.epi")) return VAE_E_BADARG;
  if (a->x_nchw_f32) return fail(VAE_E_UNSUPPORTED, "conv2d_bwd_data: no gradient for the NCHW image input");
  const int S = a->stride;
  if (a->h % S || a->w % S || a->h / S != a->p || a->w / S != a->q)
    return fail(VAE_E_BADSHAPE, "conv2d_bwd_data: needs h == p*stride (got h=%d p=%d S=%d)", a->h, a->p, S);
  hipStream_t st = (hipStream_t)stream;
  // what the VQ-VAE's tile kernels take: bf16 with the caller's swapped-axes weights, dy as
  // stored, at most a LeakyReLU backward, no BatchNorm sums
  const bool tile = a->dtype == VAE_BF16 && a->wt_t && a->dy_xf.kind == VAE_X_NONE &&
                    (a->dx_epi.kind == VAE_X_NONE || a->dx_epi.kind == VAE_X_ACT) && !a->dx_dgamma && !a->bn_finalize &&
                    a->split_k <= 0;
  // 1x1 stride 1 (the VQ-VAE ResidualLayer's Conv1x1): pixel-tile GEMM over WT[c][k]
  if (tile && pointwise(a) && p1_shape_ok((long)a->n * a->h * a->w, a->k, a->c)) {
    P1Args c;
    memset(&c, 0, sizeof(c));
    c.a = a->dy; c.b = a->wt_t; c.out = a->dx; c.residual = a->residual;
    if (a->dx_epi.kind == VAE_X_ACT) { c.aux = a->dx_epi.aux; c.aux_slope = a->dx_epi.slope; }
    c.M = (long)a->n * a->h * a->w; c.C = a->k; c.N = a->c;
    return p1_launch(c, st);
  }
  // 3x3 stride-1 on a 16 x 16 grid (the VQ-VAE's residual stacks): the image-tile kernel, taps
  // flipped, over the caller's swapped-axes weights WT[c][r][s][k]
  if (tile && c3_shape_ok(a->n, a->p, a->q, a->h, a->w, a->r, a->stride, a->pad, a->k, a->c)) {
    C3Args c;
    memset(&c, 0, sizeof(c));
    c.a = a->dy; c.b = a->wt_t; c.flip = 1; c.out = a->dx; c.residual = a->residual;
    if (a->dx_epi.kind == VAE_X_ACT) { c.aux = a->dx_epi.aux; c.aux_slope = a->dx_epi.slope; }
    c.n = a->n; c.C = a->k; c.N = a->c;
    return c3_launch(c, st);
  }
  auto epilogue = [&](GemmParams& p) {
    return bwd_epilogue(p, a->dx_epi, a->dx_dgamma, a->dx_dbeta, a->sum_reps, a->sum_rstride, a->residual, what);
  };
  // the phase gather of dy (any stride; stride 1 is one phase of R*R taps) over W[k][r][s][c]
  GemmParams p;
  const bool phases = phase_gather_params(p, a, true);
  if (phases) {
    if (int rc = epilogue(p)) return rc;
  }
  if (phases && a->dtype == VAE_BF16) {
    // bf16 conv-GEMM: against the swapped-axes weights WT[c][r][s][k] (caller's wt_t, or built at
    // the workspace's end)
    const StagedWeights w = staged_weights(a, a->wt_t);
    GemmParams q = p;
    swapped_weights(q, w.ptr);
    if (w.ptr && cg_ok(q, E_BNBWD)) {
      if (int rc = check_finalize(a->bn_finalize, what)) return rc;
      return with_staged_weights(w, a, a->k, a->c, 0, "conv2d_bwd_data weight copy", st, [&]() -> int {
        return then_finalize(cg_launch<A_CONVT, E_BNBWD>(q, a->split_k, a->workspace, w.slab_bytes, st), a->bn_finalize, st);
      });
    }
  }
  if (S == 1 && a->dtype == VAE_BF16 && a->c % 8 == 0 && a->k % 8 == 0 && a->workspace) {
    // stride 1: dx = conv(dy, W') with W'[c][r][s][k] = W[k][R-1-r][R-1-s][c] and pad R-1-P — the
    // forward conv path (k-contiguous weight rows, packed im2col gather of dy) instead of the
    // phase-gather with k-strided weights.  W' lives at the end of the workspace.
    const StagedWeights w = staged_weights(a, nullptr);
    return with_staged_weights(w, a, a->k, a->c, 1, "conv2d_bwd_data weight copy", st, [&]() -> int {
      GemmParams f = strided_conv_params(a, true, w.ptr, a->r - 1 - a->pad);
      if (int rc = epilogue(f)) return rc;
      if (int rc = check_finalize(a->bn_finalize, what)) return rc;
      return then_finalize(launch<A_CONV, B_NK, E_BNBWD, true, false>(a->dtype, false, false, f, a->split_k, a->workspace,
                                                                      w.slab_bytes, st),
                           a->bn_finalize, st);
    });
  }
  if (!phases) return fail(VAE_E_UNSUPPORTED, "conv2d_bwd_data: stride/kernel");
  if (int rc = check_finalize(a->bn_finalize, what)) return rc;
  return then_finalize(launch<A_CONVT, B_KN, E_BNBWD, true, false>(a->dtype, false, false, p, a->split_k, a->workspace,
                                                                   a->workspace_bytes, st),
                       a->bn_finalize, st);
}
