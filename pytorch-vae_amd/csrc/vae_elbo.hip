// vae_elbo_fwd: the loss of vae_elbo.hpp as a launch of its own (one workgroup).  A step that fuses
// it runs elbo_block inside the head backward's reduction or the optimizer launch instead.
#include "vae_elbo.hpp"

namespace vae {
namespace {

__global__ void __launch_bounds__(256) elbo_kernel(vae_elbo_args a) {
  kernarg_prefetch<(sizeof(vae_elbo_args) < 1024 ? sizeof(vae_elbo_args) : 1024)>();
  __shared__ float kld_row[1024];
  __shared__ float red[4][4];
  elbo_block(a, kld_row, red);
}

}  // namespace
}  // namespace vae

using namespace vae;

extern "C" int vae_elbo_fwd(const vae_elbo_args* a, void* stream) {
  if (!a || !a->sse || !a->out || !a->per_img) return fail(VAE_E_BADARG, "elbo_fwd: args");
  if (a->kind < VAE_LOSS_VANILLA || a->kind > VAE_LOSS_MIWAE) return fail(VAE_E_BADARG, "elbo_fwd: kind");
  if (a->kind == VAE_LOSS_MIWAE) {
    // (the tensors before the shapes: mmd_tiles carries the estimates M, samples the M*K rows per image)
    if (!a->mulv || !a->head_coef || !a->kl_coef) return fail(VAE_E_BADARG, "elbo_fwd: MIWAE mulv / head_coef / kl_coef");
    const int rows = a->samples > 0 ? a->samples : 1;
    if (a->mmd_tiles < 1) return fail(VAE_E_BADSHAPE, "elbo_fwd: MIWAE estimates %d below 1 (mmd_tiles)", a->mmd_tiles);
    if (rows % a->mmd_tiles)
      return fail(VAE_E_BADSHAPE, "elbo_fwd: MIWAE samples %d not a multiple of estimates %d", rows, a->mmd_tiles);
    if (a->batch < 1 || a->batch > 1024) return fail(VAE_E_BADSHAPE, "elbo_fwd: MIWAE batch %d outside 1..1024", a->batch);
  }
  if (a->kind == VAE_LOSS_DIP) {
    if (!a->mmd_partials || !a->mmd_out || a->mmd_tiles <= 0) return fail(VAE_E_BADARG, "elbo_fwd: dip partials / dip out (mmd_partials, mmd_out, mmd_tiles)");
    if (a->samples > 1) return fail(VAE_E_BADSHAPE, "elbo_fwd: DIP-VAE takes one sample");
  }
  if (a->kind == VAE_LOSS_INFO) {
    if (!a->mmd_partials || !a->mmd_out || a->mmd_tiles <= 0) return fail(VAE_E_BADARG, "elbo_fwd: mmd partials / mmd_out");
    if (a->batch < 2 || a->samples > 1) return fail(VAE_E_BADSHAPE, "elbo_fwd: InfoVAE needs batch >= 2, one sample");
  }
  if (a->kind == VAE_LOSS_VQ) {
    if (!a->vq_sse || !(a->vq_elems > 0.f)) return fail(VAE_E_BADARG, "elbo_fwd: vq_sse / vq_elems");
    if (a->batch <= 0 || a->img_elems <= 0 || (a->samples > 1)) return fail(VAE_E_BADSHAPE, "elbo_fwd: sizes");
  } else {
    if (!a->mulv || !a->head_coef || !a->kl_coef) return fail(VAE_E_BADARG, "elbo_fwd: args");
    if (a->batch <= 0 || a->batch > 1024 || a->latent <= 0 || a->img_elems <= 0) return fail(VAE_E_BADSHAPE, "elbo_fwd: sizes");
  }
  VAE_LAUNCH(elbo_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("elbo_fwd");
}
