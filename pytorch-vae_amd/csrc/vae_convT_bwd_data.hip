// C-ABI entry points of ConvTranspose2d (decoder blocks, models/vanilla_vae.py:50-55, :65-70).
#include "vae_launch.hpp"
#include "vae_wgrad.hpp"

using namespace vae;

// dx[n,h,w,c] = Σ_{r,s,k} dy'[n, h*S-P+r, w*S-P+s, k] · W[c][r][s][k]   (strided conv of dy)
extern "C" int vae_convT2d_bwd_data(const vae_conv_args* a, void* stream) {
  if (int rc = check_geom(a, "convT2d_bwd_data")) return rc;
  if (!a->dy || !a->wt || !a->dx) return fail(VAE_E_BADARG, "convT2d_bwd_data: null tensor");
  if (!xf_ok(a->dy_xf, "convT2d_bwd_data.dy") || !epi_ok(a->dx_epi, "convT2d_bwd_data.epi")) return VAE_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  GemmParams p = strided_conv_params(a, true, a->wt, a->pad);
  // (vaehip.h: `residual` adds to dx in conv2d bwd_data only; here it is the forward's input)
  if (int rc = bwd_epilogue(p, a->dx_epi, a->dx_dgamma, a->dx_dbeta, a->sum_reps, a->sum_rstride, nullptr, "convT2d_bwd_data"))
    return rc;
  if (int rc = check_finalize(a->bn_finalize, "convT2d_bwd_data")) return rc;
  if (a->dtype == VAE_BF16 && cg_ok(p, E_BNBWD))
    return then_finalize(cg_launch<A_CONV, E_BNBWD>(p, a->split_k, a->workspace, a->workspace_bytes, st), a->bn_finalize, st);
  return then_finalize(launch<A_CONV, B_NK, E_BNBWD, true, false>(a->dtype, false, false, p, a->split_k, a->workspace,
                                                                  a->workspace_bytes, st),
                       a->bn_finalize, st);
}
