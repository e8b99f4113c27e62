// C-ABI entry points of ConvTranspose2d (decoder blocks, models/vanilla_vae.py:50-55, :65-70).
#include "vae_launch.hpp"
#include "vae_wgrad.hpp"
#include "vae_hires.hpp"

using namespace vae;

// y[n,ho,wo,k] = Σ_{r,s,c: ho = h*S-P+r} xf(x)[n,h,w,c] · W[c][r][s][k] + b[k]   (phase GEMMs)
extern "C" int vae_convT2d_fwd(const vae_conv_args* a, void* stream) {
  if (int rc = check_geom(a, "convT2d_fwd")) return rc;
  if (!a->x || !a->wt || !a->y) return fail(VAE_E_BADARG, "convT2d_fwd: null tensor");
  if (!xf_ok(a->x_xf, "convT2d_fwd.x")) return VAE_E_BADARG;
  const int S = a->stride;
  if (a->p % S || a->q % S) return fail(VAE_E_BADSHAPE, "convT2d_fwd: output not a multiple of stride");
  hipStream_t st = (hipStream_t)stream;
  GemmParams p;
  if (!phase_gather_params(p, a, false)) return fail(VAE_E_UNSUPPORTED, "convT2d_fwd: stride/kernel");
  fwd_epilogue(p, a);
  if (int rc = check_finalize(a->bn_finalize, "convT2d_fwd")) return rc;
  if (a->dtype == VAE_BF16) {
    // the decoder's full-resolution last ConvTranspose2d (32 -> 32, 32x32 -> 64x64)
    const int rc = hires_convT_fwd_launch(a, st);
    if (rc != kRouteDeclined) return rc;
    // bf16 conv-GEMM: B = the swapped-axes weight copy WT[k][r][s][c] (k-contiguous rows), taken
    // from the caller (wt_t, refreshed with the weights) or built at the end of the workspace
    const StagedWeights w = staged_weights(a, a->wt_t);
    GemmParams q = p;
    swapped_weights(q, w.ptr);
    if (w.ptr && cg_ok(q, E_STORE)) {
      return with_staged_weights(w, a, a->c, a->k, 0, "convT2d_fwd weight copy", st, [&]() -> int {
        return then_finalize(cg_launch<A_CONVT, E_STORE>(q, a->split_k, a->workspace, w.slab_bytes, st), a->bn_finalize, st);
      });
    }
  }
  return then_finalize(launch<A_CONVT, B_KN, E_STORE, false, false>(a->dtype, false, false, p, a->split_k, a->workspace,
                                                                    a->workspace_bytes, st),
                       a->bn_finalize, st);
}
