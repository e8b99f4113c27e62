// C-ABI entry points of Conv2d (encoder blocks, models/vanilla_vae.py:28-29 run at :84).
#include "vae_launch.hpp"
#include "vae_wgrad.hpp"
#include "vae_c3.hpp"

using namespace vae;

// y[n,p,q,k] = Σ_{r,s,c} xf(x)[n, p*S-P+r, q*S-P+s, c] · W[k][r][s][c] + b[k]
extern "C" int vae_conv2d_fwd(const vae_conv_args* a, void* stream) {
  if (int rc = check_geom(a, "conv2d_fwd")) return rc;
  if (!a->x || !a->wt || !a->y) return fail(VAE_E_BADARG, "conv2d_fwd: null tensor");
  if (!xf_ok(a->x_xf, "conv2d_fwd.x")) return VAE_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  // what the VQ-VAE's tile kernels take: bf16 NHWC, at most a LeakyReLU on x, no statistics
  const bool tile = a->dtype == VAE_BF16 && !a->x_nchw_f32 && (a->x_xf.kind == VAE_X_NONE || a->x_xf.kind == VAE_X_ACT) &&
                    !a->y_sum && !a->y_sumsq && !a->bn_finalize && a->split_k <= 0;
  // 1x1 stride-1 convs (the VQ-VAE ResidualLayer's Conv1x1 + skip add): pixel-tile kernel
  if (tile && pointwise(a) && p1_shape_ok((long)a->n * a->p * a->q, a->c, a->k) &&
      (a->residual_xf.kind == VAE_X_NONE || a->residual_xf.kind == VAE_X_ACT)) {
    P1Args c;
    memset(&c, 0, sizeof(c));
    c.a = a->x; c.a_act = a->x_xf.kind == VAE_X_ACT; c.a_slope = a->x_xf.slope;
    c.b = a->wt; c.out = a->y; c.bias = a->bias;
    c.residual = a->residual; c.res_act = a->residual && a->residual_xf.kind == VAE_X_ACT; c.res_slope = a->residual_xf.slope;
    c.M = (long)a->n * a->p * a->q; c.C = a->c; c.N = a->k;
    return p1_launch(c, st);
  }
  // 3x3 stride-1 convs on a 16 x 16 grid (the VQ-VAE's residual stacks): image-tile kernel
  if (tile && c3_shape_ok(a->n, a->h, a->w, a->p, a->q, a->r, a->stride, a->pad, a->c, a->k) && !a->residual) {
    C3Args c;
    memset(&c, 0, sizeof(c));
    c.a = a->x; c.a_act = a->x_xf.kind == VAE_X_ACT; c.a_slope = a->x_xf.slope;
    c.b = a->wt; c.flip = 0; c.out = a->y; c.bias = a->bias;
    c.n = a->n; c.C = a->c; c.N = a->k;
    return c3_launch(c, st);
  }
  GemmParams p = strided_conv_params(a, false, a->wt, a->pad);
  fwd_epilogue(p, a);
  if (int rc = check_finalize(a->bn_finalize, "conv2d_fwd")) return rc;
  if (a->dtype == VAE_BF16 && cg_ok(p, E_STORE))
    return then_finalize(cg_launch<A_CONV, E_STORE>(p, a->split_k, a->workspace, a->workspace_bytes, st), a->bn_finalize, st);
  return then_finalize(launch<A_CONV, B_NK, E_STORE, false, false, true>(a->dtype, a->x_nchw_f32 != 0, false, p, a->split_k,
                                                                         a->workspace, a->workspace_bytes, st),
                       a->bn_finalize, st);
}
