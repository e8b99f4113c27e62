// Launcher of the decoder's full-resolution last ConvTranspose2d forward (vae_hires.hip).  Returns
// kRouteDeclined when the call is not the shape / transform its kernel takes.
#pragma once
#include "vae_common.hpp"

namespace vae {
int hires_convT_fwd_launch(const vae_conv_args* a, hipStream_t st);
}  // namespace vae
