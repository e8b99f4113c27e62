// vae_step_begin_ex: the head of a training step as ONE launch (vaehip.h).  Three kinds of work that
// do not depend on each other share the grid as block ranges:
//   [0, nz)            zero the step's zero region (gradients, BatchNorm sums, SSE, d[mu|logvar]) and
//                      ++*step — vae_step_begin
//   [nz, nz + nx)      the fp32 NCHW image -> NHWC with cp channels (zeros above c), one pixel per
//                      thread, one 16-byte store per pixel for bf16 / cp = 8 — vae_nchw_to_nhwc_pad
//   [nz + nx, ...)     up to VAE_PAD_MAX padded weight copies — vae_pad_channels
//   [..., end)         up to VAE_SWAP_MAX swapped-axes weight copies — vae_swap_axes (they read the fp32
//                      weights the previous step's optimizer wrote; measured as a launch of their own
//                      behind the optimizer: 8.5 us per VanillaVAE step, profiles/r5p)
// The reference's step (experiment.py:45-49) feeds the image straight into the first Conv2d
// (models/vanilla_vae.py:84); the padding exists only so that the first layer runs on the packed
// 16-byte GEMM operand path.  profiles/r3a: the three separate launches took 6.5 + 5.2 + 4.8 us.
//
// The stand-alone forms of its ranges live here too (vae_step_begin, vae_swap_axes), and the tail
// of the step: vae_step_record.
#include <algorithm>

#include <math.h>

#include "vae_common.hpp"

namespace vae {
namespace {

constexpr int kZeroRanges = VAE_SLAB_MAX + 1;
struct StepBegin {
  vae_step_begin_args a;
  long n16;              // 16-byte words of the zero region
  int ntail;             // bytes after them
  int nz, nx;            // blocks of the zeroing and of the image ranges
  int nzr;                          // zeroed ranges (the region minus its keep ranges)
  int zb0[kZeroRanges + 1];         // first block of each range
  long zoff[kZeroRanges], zlen[kZeroRanges];   // in 16-byte words
  int pad0[VAE_PAD_MAX + 1];   // first block of each pad descriptor (relative to nz + nx)
  int np;                      // blocks of the pad range
  int swap0[VAE_SWAP_MAX + 1]; // first block of each swap descriptor (relative to nz + nx + np)
};

template <class T>
__device__ __forceinline__ void image_pixel(const vae_step_begin_args& a, long pix) {
  const long hw = (long)a.h * a.w;
  const long img = pix / hw, sp = pix - img * hw;
  const float* src = a.x + img * a.c * hw + sp;
  T* dst = static_cast<T*>(a.y) + pix * a.cp;
  if constexpr (sizeof(T) == 2) {
    if (a.cp == 8) {                       // the packed RGB case: one 16-byte store
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (__bf16)(j < a.c ? src[j * hw] : 0.f);
      *reinterpret_cast<bf16x8*>(dst) = o;
      return;
    }
  }
  for (int j = 0; j < a.cp; ++j) dst[j] = cvt<T>(j < a.c ? src[j * hw] : 0.f);
}

template <class T>
__global__ void __launch_bounds__(256) step_begin_ex_kernel(const StepBegin s) {
  kernarg_prefetch<(sizeof(StepBegin) < 1024 ? sizeof(StepBegin) : 1024)>();
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b < s.nz) {
    f32x4* z = static_cast<f32x4*>(s.a.zero);
    int k = 0;
    while (k + 1 < s.nzr && b >= s.zb0[k + 1]) ++k;
    const int lb = b - s.zb0[k], nb = s.zb0[k + 1] - s.zb0[k];
    f32x4* zr = z + s.zoff[k];
    for (long i = (long)lb * 256 + tid; i < s.zlen[k]; i += (long)nb * 256) zr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (b == 0 && tid < s.ntail) reinterpret_cast<unsigned char*>(z + s.n16)[tid] = 0;
    if (b == 0 && tid == 0 && s.a.step) *s.a.step += 1;
    return;
  }
  if (b < s.nz + s.nx) {
    const long pix = (long)(b - s.nz) * 256 + tid;
    if (pix < (long)s.a.n * s.a.h * s.a.w) image_pixel<T>(s.a, pix);
    return;
  }
  const int pb = b - s.nz - s.nx;
  if (pb >= s.np) {
    __shared__ float t[kSwapT][kSwapT + 1];
    const int sb = pb - s.np;
    int k = 0;
    while (k + 1 < s.a.nswap && sb >= s.swap0[k + 1]) ++k;
    swap_tile(s.a.swap[k], sb - s.swap0[k], t);
    return;
  }
  int k = 0;
  while (k + 1 < s.a.npad && pb >= s.pad0[k + 1]) ++k;
  const vae_pad_desc& d = s.a.pad[k];
  const long i = (long)(pb - s.pad0[k]) * 256 + tid;
  if (i >= d.rows * d.cp) return;
  const long r = i / d.cp;
  const int j = (int)(i - r * d.cp);
  static_cast<T*>(d.dst)[i] = j < d.c ? static_cast<const T*>(d.src)[r * d.c + j] : cvt<T>(0.f);
}

// vae_step_begin: the zeroing range alone
__global__ void step_begin_kernel(f32x4* z, long n16, unsigned char* tail, int ntail, int* step) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x)
    z[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (blockIdx.x == 0 && threadIdx.x < ntail) tail[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && step) *step += 1;
}

}  // namespace
}  // namespace vae

using namespace vae;

extern "C" int vae_step_begin(void* zero, int64_t bytes, int32_t* step, void* stream) {
  if (bytes < 0 || (bytes > 0 && !zero)) return fail(VAE_E_BADARG, "step_begin: args");
  if (((uintptr_t)zero & 15) != 0) return fail(VAE_E_BADARG, "step_begin: zero region must be 16-B aligned");
  const long n16 = bytes / 16;
  const int ntail = (int)(bytes - n16 * 16);
  VAE_LAUNCH(step_begin_kernel, dim3(grid_for(n16 > 0 ? n16 : 1)), dim3(256), 0, (hipStream_t)stream,
                     (f32x4*)zero, n16, (unsigned char*)zero + n16 * 16, ntail, (int*)step);
  return check_launch("step_begin");
}

extern "C" int vae_step_begin_ex(const vae_step_begin_args* a, void* stream) {
  if (!a || a->bytes < 0 || (a->bytes > 0 && !a->zero)) return fail(VAE_E_BADARG, "step_begin_ex: zero region");
  if (((uintptr_t)a->zero & 15) != 0) return fail(VAE_E_BADARG, "step_begin_ex: zero region must be 16-B aligned");
  if (a->dtype != VAE_F32 && a->dtype != VAE_BF16) return fail(VAE_E_BADDTYPE, "step_begin_ex: dtype");
  if (a->npad < 0 || a->npad > VAE_PAD_MAX) return fail(VAE_E_BADARG, "step_begin_ex: %d pads", a->npad);
  StepBegin s;
  s.a = *a;
  s.n16 = a->bytes / 16;
  s.ntail = (int)(a->bytes - s.n16 * 16);
  // the zeroed ranges: the region minus its keep ranges (sorted, clipped, 16-byte words inward)
  if (a->nkeep < 0 || a->nkeep > VAE_SLAB_MAX) return fail(VAE_E_BADARG, "step_begin_ex: %d keep ranges", a->nkeep);
  long ko[VAE_SLAB_MAX], ke[VAE_SLAB_MAX];
  int nk = 0;
  for (int k = 0; k < a->nkeep; ++k) {
    const long o = (a->keep[k].off + 15) / 16, e = (a->keep[k].off + a->keep[k].bytes) / 16;
    if (a->keep[k].off < 0 || a->keep[k].bytes < 0) return fail(VAE_E_BADARG, "step_begin_ex: keep %d", k);
    const long oo = o < s.n16 ? o : s.n16, ee = e < s.n16 ? e : s.n16;
    if (ee > oo) { ko[nk] = oo; ke[nk] = ee; ++nk; }
  }
  std::sort(ko, ko + nk);
  std::sort(ke, ke + nk);              // (keep ranges do not overlap: the gradients of distinct tensors)
  s.nzr = 0;
  long pos = 0;
  for (int k = 0; k <= nk; ++k) {
    const long end = k < nk ? ko[k] : s.n16;
    if (end > pos) { s.zoff[s.nzr] = pos; s.zlen[s.nzr] = end - pos; ++s.nzr; }
    if (k < nk && ke[k] > pos) pos = ke[k];
  }
  if (s.nzr == 0) { s.zoff[0] = 0; s.zlen[0] = 0; s.nzr = 1; }
  int zb = 0;
  for (int k = 0; k < s.nzr; ++k) {
    s.zb0[k] = zb;
    const long nb = (s.zlen[k] + 255) / 256;
    zb += (int)(nb < 1 ? 1 : (nb > 2048 ? 2048 : nb));
  }
  s.zb0[s.nzr] = zb;
  s.nz = zb;
  s.nx = 0;
  if (a->x) {
    if (!a->y || a->n <= 0 || a->c <= 0 || a->h <= 0 || a->w <= 0 || a->cp < a->c)
      return fail(VAE_E_BADARG, "step_begin_ex: image args");
    if (a->dtype == VAE_BF16 && a->cp == 8 && ((uintptr_t)a->y & 15) != 0)
      return fail(VAE_E_BADARG, "step_begin_ex: padded image must be 16-B aligned");
    s.nx = (int)(((long)a->n * a->h * a->w + 255) / 256);
  }
  int nb = 0;
  for (int k = 0; k < a->npad; ++k) {
    const vae_pad_desc& d = a->pad[k];
    if (!d.src || !d.dst || d.rows <= 0 || d.c <= 0 || d.cp < d.c) return fail(VAE_E_BADARG, "step_begin_ex: pad %d", k);
    s.pad0[k] = nb;
    nb += (int)((d.rows * d.cp + 255) / 256);
  }
  s.pad0[a->npad] = nb;
  s.np = nb;
  if (a->nswap < 0 || a->nswap > VAE_SWAP_MAX) return fail(VAE_E_BADARG, "step_begin_ex: %d swaps", a->nswap);
  int ns = 0;
  for (int k = 0; k < a->nswap; ++k) {
    const vae_swap_desc& d = a->swap[k];
    if (!d.src || !d.dst || d.a <= 0 || d.b <= 0 || d.rs <= 0 || (d.src_dtype != VAE_F32 && d.src_dtype != VAE_BF16))
      return fail(VAE_E_BADARG, "step_begin_ex: swap %d", k);
    s.swap0[k] = ns;
    ns += swap_tiles(d);
  }
  s.swap0[a->nswap] = ns;
  const dim3 grid((unsigned)(s.nz + s.nx + nb + ns));
  if (a->dtype == VAE_BF16) VAE_LAUNCH(step_begin_ex_kernel<__bf16>, grid, dim3(256), 0, (hipStream_t)stream, s);
  else VAE_LAUNCH(step_begin_ex_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, s);
  return check_launch("step_begin_ex");
}

// ------------------------------------------------------------------ training-step record
namespace {
__global__ void __launch_bounds__(256) step_record_kernel(const vae_record_args a) {
  kernarg_prefetch<(sizeof(vae_record_args) < 1024 ? sizeof(vae_record_args) : 1024)>();
  __shared__ float pv[1024];
  __shared__ float rv[2][256];
  __shared__ int ri[2][256];
  __shared__ int win[2];
  const int tid = threadIdx.x;
  if (tid < a.nterms) a.terms[tid] = a.src_terms[tid];
  const float inv_s = 1.0f / (float)a.samples;
  for (int b = tid; b < a.batch; b += 256) {
    float v = 0.f;
    for (int s = 0; s < a.samples; ++s) v += a.per_img[b * a.samples + s];
    v *= inv_s;
    pv[b] = v;
    a.per[b] = v;
  }
  __syncthreads();
  // first index of the maximum / minimum (ties -> lowest index, as the reference's strict '>'/'<')
  float mx = -INFINITY, mn = INFINITY;
  int imx = 0x7fffffff, imn = 0x7fffffff;
  for (int b = tid; b < a.batch; b += 256) {
    const float v = pv[b];
    if (v > mx) { mx = v; imx = b; }
    if (v < mn) { mn = v; imn = b; }
  }
  rv[0][tid] = mx; ri[0][tid] = imx; rv[1][tid] = mn; ri[1][tid] = imn;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      const float v1 = rv[0][tid + off], v0 = rv[0][tid];
      const int i1 = ri[0][tid + off], i0 = ri[0][tid];
      if (v1 > v0 || (v1 == v0 && i1 < i0)) { rv[0][tid] = v1; ri[0][tid] = i1; }
      const float w1 = rv[1][tid + off], w0 = rv[1][tid];
      const int j1 = ri[1][tid + off], j0 = ri[1][tid];
      if (w1 < w0 || (w1 == w0 && j1 < j0)) { rv[1][tid] = w1; ri[1][tid] = j1; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    win[0] = rv[0][0] > a.best[0] ? ri[0][0] : -1;
    win[1] = rv[1][0] < a.best[1] ? ri[1][0] : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int b = win[k];
    if (b < 0) continue;
    float* di = k == 0 ? a.hi_img : a.lo_img;
    float* dr = k == 0 ? a.hi_recon : a.lo_recon;
    for (int e = tid; e < a.img_elems; e += 256) {
      di[e] = a.img[(long)b * a.img_elems + e];
      dr[e] = a.recon[(long)b * a.samples * a.img_elems + e];
    }
    if (tid == 0) { a.best[k] = rv[k][0]; a.at[2 * k] = a.step; a.at[2 * k + 1] = b; }
  }
}
}  // namespace

extern "C" int vae_step_record(const vae_record_args* a, void* stream) {
  if (!a || a->batch <= 0 || a->batch > 1024 || a->samples <= 0 || a->img_elems <= 0 || a->nterms < 0 || a->nterms > 8 ||
      (a->nterms && (!a->src_terms || !a->terms)) || !a->per_img || !a->per || !a->img || !a->recon || !a->best || !a->at ||
      !a->hi_img || !a->hi_recon || !a->lo_img || !a->lo_recon)
    return fail(VAE_E_BADARG, "step_record: args");
  VAE_LAUNCH(step_record_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("step_record");
}

// ------------------------------------------------------------------ swapped-axes weight copies
// dst[b][t][a] = bf16(src[a][t][b]) for up to VAE_SWAP_MAX tensors in one launch: the k-contiguous
// B operands of the bf16 ConvTranspose2d forward / Conv2d data-gradient GEMMs (vaehip.h wt_t),
// refreshed from the fp32 master right after the optimizer step.  One workgroup = one
// kSwapT x kSwapT (64x64) (a, b) tile of one tap through a padded LDS tile, each lane moving an
// element pair (swap_tile, vae_common.hpp).
namespace {
struct SwapBatch {
  vae_swap_desc d[VAE_SWAP_MAX];
  int tiles0[VAE_SWAP_MAX + 1];      // first workgroup of each descriptor
  int count;
};

__global__ void __launch_bounds__(256) swap_axes_kernel(const SwapBatch sb) {
  kernarg_prefetch<(sizeof(SwapBatch) < 1024 ? sizeof(SwapBatch) : 1024)>();
  __shared__ float t[kSwapT][kSwapT + 1];
  int i = 0;
  while (i + 1 < sb.count && (int)blockIdx.x >= sb.tiles0[i + 1]) ++i;
  swap_tile(sb.d[i], blockIdx.x - sb.tiles0[i], t);
}
}  // namespace

extern "C" int vae_swap_axes(int32_t count, const vae_swap_desc* descs, void* stream) {
  if (count <= 0) return VAE_OK;
  if (count > VAE_SWAP_MAX || !descs) return fail(VAE_E_BADARG, "swap_axes: count %d (max %d)", count, VAE_SWAP_MAX);
  SwapBatch sb;
  memset(&sb, 0, sizeof(sb));
  int tiles = 0;
  for (int i = 0; i < count; ++i) {
    const vae_swap_desc& d = descs[i];
    if (!d.src || !d.dst || d.a <= 0 || d.b <= 0 || d.rs <= 0 || (d.src_dtype != VAE_F32 && d.src_dtype != VAE_BF16))
      return fail(VAE_E_BADARG, "swap_axes: descriptor %d", i);
    sb.d[i] = d;
    sb.tiles0[i] = tiles;
    tiles += swap_tiles(d);
  }
  sb.tiles0[count] = tiles;
  sb.count = count;
  VAE_LAUNCH(swap_axes_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, sb);
  return check_launch("swap_axes");
}
