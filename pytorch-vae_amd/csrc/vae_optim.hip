// The optimizer step (torch.optim.Adam's single-tensor update) over the flat parameter buffer:
// vae_adam_step, vae_adam_step_ex (the same update with the backward's deferred weight-gradient
// reductions and loss in its grid), vae_grad_sumsq + vae_adam_step_clip (the update under
// clip_grad_norm_: the gradient's sum of squares, then Adam with the clip coefficient folded in) and
// vae_cast_bf16 (the bf16 parameter copy).
#include <algorithm>

#include <math.h>

#include "vae_common.hpp"
#include "vae_elbo.hpp"

namespace vae {
namespace {

// ---------------------------------------------------------------------------- Adam
struct AdamK {
  float omb1, omb2, b2f, step_size, bc2s, eps, wd;
};
__device__ __forceinline__ float adam_elem(const AdamK& k, float& pi, float gi, float& mi, float& vi) {
  if (k.wd != 0.f) gi = fmaf(k.wd, pi, gi);
  mi = mi + k.omb1 * (gi - mi);                                      // lerp (torch Adam)
  vi = vi * k.b2f + k.omb2 * gi * gi;                                // mul_(beta2).addcmul_(g, g, 1-beta2)
  const float den = sqrtf(vi) / k.bc2s + k.eps;
  pi = pi - k.step_size * (mi / den);
  return pi;
}
// V = 4: 16-byte accesses (the four fp32 arrays 16-byte aligned, the bf16 copy 8-byte aligned),
// the n % 4 tail by block 0; V = 1: one element per access
template <bool LOWP, int V>
__global__ void __launch_bounds__(256) adam_kernel(long n, float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, const int* step,
                                                   const float* lr, double b1, double b2, float eps, float wd,
                                                   __bf16* __restrict__ lowp) {
  // torch.optim.Adam (single-tensor path): the scalars it derives from the Python-float
  // hyper-parameters (1 - beta, bias corrections, step size) are formed in double and rounded
  // once, as torch does — 1 - 0.999f in fp32 would be 1.3e-5 off 1 - 0.999
  const double t = (double)(*step);
  const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
  const AdamK k{(float)(1.0 - b1), (float)(1.0 - b2), (float)b2, (float)((double)*lr / bc1), (float)sqrt(bc2), eps, wd};
  const long stride = (long)gridDim.x * blockDim.x;
  const long nv = n / V;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    if constexpr (V == 4) {
      f32x4 p4 = reinterpret_cast<const f32x4*>(p)[i];
      const f32x4 g4 = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 m4 = reinterpret_cast<const f32x4*>(m)[i];
      f32x4 v4 = reinterpret_cast<const f32x4*>(v)[i];
      float pe[4], me[4], ve[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pe[e] = p4[e]; me[e] = m4[e]; ve[e] = v4[e];
        adam_elem(k, pe[e], g4[e], me[e], ve[e]);
      }
      reinterpret_cast<f32x4*>(p)[i] = f32x4{pe[0], pe[1], pe[2], pe[3]};
      reinterpret_cast<f32x4*>(m)[i] = f32x4{me[0], me[1], me[2], me[3]};
      reinterpret_cast<f32x4*>(v)[i] = f32x4{ve[0], ve[1], ve[2], ve[3]};
      if (LOWP) reinterpret_cast<bf16x4*>(lowp)[i] = bf16x4{(__bf16)pe[0], (__bf16)pe[1], (__bf16)pe[2], (__bf16)pe[3]};
    } else {
      float pi = p[i], mi = m[i], vi = v[i];
      adam_elem(k, pi, g[i], mi, vi);
      m[i] = mi; v[i] = vi; p[i] = pi;
      if (LOWP) lowp[i] = (__bf16)pi;
    }
  }
  if (V > 1 && blockIdx.x == 0 && threadIdx.x < n - nv * V) {
    const long i = nv * V + threadIdx.x;
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(k, pi, g[i], mi, vi);
    m[i] = mi; v[i] = vi; p[i] = pi;
    if (LOWP) lowp[i] = (__bf16)pi;
  }
}

// ---------------------------------------------------------------------------- gradient-norm clip
// vae_grad_sumsq: workgroup b sums g[i]^2 over the contiguous range of quads (V = 4) or elements
// (V = 1) that n and the grid alone assign to it — thread t takes t, t + 256, ... in ascending order,
// products and sums in double (a product of two floats is exact in double) — then the 64 lanes of a
// wave combine by shuffles and the four waves in LDS, in a fixed order: partials[b] is the same bits
// at every run.  No atomics; the n % 4 tail goes to workgroup 0.
constexpr int kSumsqPer = 4096;        // elements per workgroup before the grid reaches its cap
inline int sumsq_parts(long n) {
  const long b = (n + kSumsqPer - 1) / kSumsqPer;
  return (int)std::min<long>(std::max<long>(b, 1), VAE_SUMSQ_MAX_PARTS);
}
template <int V>
__global__ void __launch_bounds__(256) grad_sumsq_kernel(long n, const float* __restrict__ g,
                                                         double* __restrict__ partials) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long nv = n / V;
  const long chunk = (nv + gridDim.x - 1) / gridDim.x;
  const long lo = (long)blockIdx.x * chunk;
  const long hi = lo + chunk < nv ? lo + chunk : nv;
  double acc = 0.0;
  auto add = [&](float x) { acc = fma((double)x, (double)x, acc); };
  long i = lo + tid;
  if constexpr (V == 4) {
    // four 16-byte loads in flight per thread, added in the order they were issued
    for (; i + 3 * 256 < hi; i += 4 * 256) {
      f32x4 t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t[u] = reinterpret_cast<const f32x4*>(g)[i + 256 * u];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) add(t[u][e]);
    }
    for (; i < hi; i += 256) {
      const f32x4 t = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) add(t[e]);
    }
    if (blockIdx.x == 0 && tid < n - nv * V) add(g[nv * V + tid]);
  } else {
    for (; i < hi; i += 256) add(g[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// The clip coefficient of torch.nn.utils.clip_grad_norm_ (L2 norm, error_if_nonfinite=False) from
// vae_grad_sumsq's partials, by all 256 threads of a workgroup: thread t adds partials t, t + 256,
// ... in ascending order, an LDS tree adds the 256 sums — the same order in every workgroup, so all
// of them hold the bit-identical total and coefficient.  A NaN norm gives a NaN coefficient and an
// infinite one 0, as torch.clamp(max_norm / (total + 1e-6), max=1.0) does.
__device__ __forceinline__ float clip_coef(const double* __restrict__ partials, int nparts, const float* max_norm,
                                           float* norm_out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < nparts; i += 256) s += partials[i];
  red[tid] = s;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const float total = (float)sqrt(red[0]);
  const float c = *max_norm / (total + 1e-6f);
  const float coef = c > 1.f ? 1.f : c;
  if (blockIdx.x == 0 && tid == 0) {
    norm_out[0] = total;
    norm_out[1] = coef;
  }
  return coef;
}

// adam_kernel with every gradient element multiplied by the clip coefficient first (one fp32
// multiply, never contracted into the update; g is only read).  A sibling, not a template parameter
// of adam_kernel: sharing the body through an inlined helper moved adam_kernel's register allocation,
// and the unclipped kernel is on every benched path.
template <bool LOWP, int V>
__global__ void __launch_bounds__(256) adam_clip_kernel(long n, float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, const int* step,
                                                        const float* lr, double b1, double b2, float eps, float wd,
                                                        __bf16* __restrict__ lowp, const double* __restrict__ partials,
                                                        int nparts, const float* max_norm, float* norm_out) {
  const float coef = clip_coef(partials, nparts, max_norm, norm_out);
  const double t = (double)(*step);
  const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
  const AdamK k{(float)(1.0 - b1), (float)(1.0 - b2), (float)b2, (float)((double)*lr / bc1), (float)sqrt(bc2), eps, wd};
  const long stride = (long)gridDim.x * blockDim.x;
  const long nv = n / V;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    if constexpr (V == 4) {
      f32x4 p4 = reinterpret_cast<const f32x4*>(p)[i];
      const f32x4 g4 = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 m4 = reinterpret_cast<const f32x4*>(m)[i];
      f32x4 v4 = reinterpret_cast<const f32x4*>(v)[i];
      float pe[4], me[4], ve[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pe[e] = p4[e]; me[e] = m4[e]; ve[e] = v4[e];
        adam_elem(k, pe[e], __fmul_rn(g4[e], coef), me[e], ve[e]);
      }
      reinterpret_cast<f32x4*>(p)[i] = f32x4{pe[0], pe[1], pe[2], pe[3]};
      reinterpret_cast<f32x4*>(m)[i] = f32x4{me[0], me[1], me[2], me[3]};
      reinterpret_cast<f32x4*>(v)[i] = f32x4{ve[0], ve[1], ve[2], ve[3]};
      if (LOWP) reinterpret_cast<bf16x4*>(lowp)[i] = bf16x4{(__bf16)pe[0], (__bf16)pe[1], (__bf16)pe[2], (__bf16)pe[3]};
    } else {
      float pi = p[i], mi = m[i], vi = v[i];
      adam_elem(k, pi, __fmul_rn(g[i], coef), mi, vi);
      m[i] = mi; v[i] = vi; p[i] = pi;
      if (LOWP) lowp[i] = (__bf16)pi;
    }
  }
  if (V > 1 && blockIdx.x == 0 && threadIdx.x < n - nv * V) {
    const long i = nv * V + threadIdx.x;
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(k, pi, __fmul_rn(g[i], coef), mi, vi);
    m[i] = mi; v[i] = vi; p[i] = pi;
    if (LOWP) lowp[i] = (__bf16)pi;
  }
}

__global__ void cast_bf16_kernel(long n, const float* src, __bf16* dst) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dst[i] = (__bf16)src[i];
}

}  // namespace
}  // namespace vae

using namespace vae;

extern "C" int vae_adam_step(int64_t n, float* p, const float* g, float* m, float* v, const int32_t* step,
                             const float* lr, double beta1, double beta2, float eps, float weight_decay, void* p_lowp,
                             void* stream) {
  if (n <= 0) return VAE_OK;
  if (!p || !g || !m || !v || !step || !lr) return fail(VAE_E_BADARG, "adam_step: null");
  auto al = [](const void* q, uintptr_t a) { return ((uintptr_t)q % a) == 0; };
  const bool vec = al(p, 16) && al(g, 16) && al(m, 16) && al(v, 16) && (!p_lowp || al(p_lowp, 8));
  const hipStream_t st = (hipStream_t)stream;
  __bf16* lp = (__bf16*)p_lowp;
  if (vec) {
    const int grid = grid_for((n + 3) / 4);
    if (p_lowp) VAE_LAUNCH((adam_kernel<true, 4>), dim3(grid), dim3(256), 0, st, (long)n, p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, lp);
    else VAE_LAUNCH((adam_kernel<false, 4>), dim3(grid), dim3(256), 0, st, (long)n, p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, lp);
  } else {
    const int grid = grid_for(n);
    if (p_lowp) VAE_LAUNCH((adam_kernel<true, 1>), dim3(grid), dim3(256), 0, st, (long)n, p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, lp);
    else VAE_LAUNCH((adam_kernel<false, 1>), dim3(grid), dim3(256), 0, st, (long)n, p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, lp);
  }
  return check_launch("adam_step");
}

extern "C" int vae_grad_sumsq(int64_t n, const float* g, double* partials, int32_t* nparts_out, void* stream) {
  if (!nparts_out) return fail(VAE_E_BADARG, "grad_sumsq: nparts_out");
  *nparts_out = 0;
  if (n <= 0) return VAE_OK;
  if (!g || !partials) return fail(VAE_E_BADARG, "grad_sumsq: null");
  if ((uintptr_t)partials % 8) return fail(VAE_E_BADARG, "grad_sumsq: partials must be 8-byte aligned");
  const int parts = sumsq_parts(n);
  const hipStream_t st = (hipStream_t)stream;
  if ((uintptr_t)g % 16 == 0) VAE_LAUNCH(grad_sumsq_kernel<4>, dim3(parts), dim3(256), 0, st, (long)n, g, partials);
  else VAE_LAUNCH(grad_sumsq_kernel<1>, dim3(parts), dim3(256), 0, st, (long)n, g, partials);
  *nparts_out = parts;
  return check_launch("grad_sumsq");
}

extern "C" int vae_adam_step_clip(int64_t n, float* p, const float* g, float* m, float* v, const int32_t* step,
                                  const float* lr, double beta1, double beta2, float eps, float weight_decay,
                                  void* p_lowp, const double* partials, int32_t nparts, const float* max_norm,
                                  float* norm_out, void* stream) {
  if (n <= 0) return VAE_OK;
  if (!p || !g || !m || !v || !step || !lr || !partials || !max_norm || !norm_out)
    return fail(VAE_E_BADARG, "adam_step_clip: null");
  if (nparts < 1 || nparts > VAE_SUMSQ_MAX_PARTS) return fail(VAE_E_BADARG, "adam_step_clip: %d partials", nparts);
  auto al = [](const void* q, uintptr_t a) { return ((uintptr_t)q % a) == 0; };
  if (!al(partials, 8)) return fail(VAE_E_BADARG, "adam_step_clip: partials must be 8-byte aligned");
  const bool vec = al(p, 16) && al(g, 16) && al(m, 16) && al(v, 16) && (!p_lowp || al(p_lowp, 8));
  const hipStream_t st = (hipStream_t)stream;
  __bf16* lp = (__bf16*)p_lowp;
  const int grid = vec ? grid_for((n + 3) / 4) : grid_for(n);
#define VAE_CLIP_LAUNCH(LOWP, V)                                                                                  \
  VAE_LAUNCH((adam_clip_kernel<LOWP, V>), dim3(grid), dim3(256), 0, st, (long)n, p, g, m, v, step, lr, beta1, beta2, \
             eps, weight_decay, lp, partials, (int)nparts, max_norm, norm_out)
  if (vec) {
    if (p_lowp) VAE_CLIP_LAUNCH(true, 4);
    else VAE_CLIP_LAUNCH(false, 4);
  } else {
    if (p_lowp) VAE_CLIP_LAUNCH(true, 1);
    else VAE_CLIP_LAUNCH(false, 1);
  }
#undef VAE_CLIP_LAUNCH
  return check_launch("adam_step_clip");
}

namespace {

// vae_adam_step_ex in one grid (the slab workgroups first: dispatched first, their longer
// reductions overlap the streaming of the plain elements instead of trailing it):
//   [0, nslabblk)             per descriptor: "tall" slabs (rows >= kTallRows: the head's and the
//                             full-resolution ConvT's per-workgroup partials) as 16 columns x 16 row
//                             parts per workgroup, parts combined in LDS in ascending order; "short"
//                             slabs (K slices of the grouped weight gradients) as 256 quads per
//                             workgroup, each thread summing its quad's rows in ascending order —
//                             then g = that sum is written and the element's Adam update runs
//   [nslabblk]                the deferred loss (elbo_block), when present
//   [.., + nreg)              vae_adam_step over the elements no descriptor covers (grid-stride,
//                             16-byte accesses; quads inside a descriptor's range are skipped)
constexpr int kTallRows = 64;
struct AdamEx {
  long n;
  float* p; float* g; float* m; float* v;
  const int* step; const float* lr;
  double b1, b2;
  float eps, wd;
  __bf16* lowp;
  int nreg, nslab;
  int tall[VAE_SLAB_MAX];
  int blk0[VAE_SLAB_MAX + 1];        // first workgroup of each descriptor, relative to nreg
  long q0[VAE_SLAB_MAX], q1[VAE_SLAB_MAX];   // quads [q0, q1) of g a descriptor covers (ascending q0)
  long off[VAE_SLAB_MAX];            // element offset of dst in g
  vae_grad_slab s[VAE_SLAB_MAX];
  int has_elbo;
  vae_elbo_args e;
};

__device__ __forceinline__ AdamK adam_k(const AdamEx& a) {
  const double t = (double)(*a.step);
  const double bc1 = 1.0 - pow(a.b1, t), bc2 = 1.0 - pow(a.b2, t);
  return AdamK{(float)(1.0 - a.b1), (float)(1.0 - a.b2), (float)a.b2, (float)((double)*a.lr / bc1), (float)sqrt(bc2),
               a.eps, a.wd};
}

template <bool LOWP>
__device__ __forceinline__ void adam_one(const AdamEx& a, const AdamK& k, long i, float gi) {
  float pi = a.p[i], mi = a.m[i], vi = a.v[i];
  adam_elem(k, pi, gi, mi, vi);
  a.m[i] = mi; a.v[i] = vi; a.p[i] = pi;
  if (LOWP) a.lowp[i] = (__bf16)pi;
}

template <bool LOWP>
__device__ __forceinline__ void adam_quad(const AdamEx& a, const AdamK& k, long i, const f32x4 g4) {
  f32x4 p4 = reinterpret_cast<const f32x4*>(a.p)[i];
  f32x4 m4 = reinterpret_cast<const f32x4*>(a.m)[i];
  f32x4 v4 = reinterpret_cast<const f32x4*>(a.v)[i];
  float pe[4], me[4], ve[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    pe[e] = p4[e]; me[e] = m4[e]; ve[e] = v4[e];
    adam_elem(k, pe[e], g4[e], me[e], ve[e]);
  }
  reinterpret_cast<f32x4*>(a.p)[i] = f32x4{pe[0], pe[1], pe[2], pe[3]};
  reinterpret_cast<f32x4*>(a.m)[i] = f32x4{me[0], me[1], me[2], me[3]};
  reinterpret_cast<f32x4*>(a.v)[i] = f32x4{ve[0], ve[1], ve[2], ve[3]};
  if (LOWP) reinterpret_cast<bf16x4*>(a.lowp)[i] = bf16x4{(__bf16)pe[0], (__bf16)pe[1], (__bf16)pe[2], (__bf16)pe[3]};
}

// (a streaming kernel: <= 64 VGPRs keeps 8 waves per SIMD; at 104 it ran 4 and took 33 us for the
// 19.6 us of bytes of vae_adam_step plus the slabs)
template <bool LOWP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) adam_ex_kernel(const AdamEx ka) {
  kernarg_prefetch<1024>();
  // fields read in place (a runtime descriptor index would copy the by-value block to scratch)
  (void)ka;
  const AdamEx& a = *(const AdamEx*)(const void*)__builtin_amdgcn_kernarg_segment_ptr();
  const int tid = threadIdx.x;
  const int nslabblk = a.blk0[a.nslab];
  if (a.has_elbo && (int)blockIdx.x == nslabblk) {
    __shared__ float kld_row[1024];
    __shared__ float ered[4][4];
    elbo_block(a.e, kld_row, ered);
    return;
  }
  const AdamK k = adam_k(a);
  if ((int)blockIdx.x >= nslabblk) {
    const int b = (int)blockIdx.x - nslabblk - (a.has_elbo ? 1 : 0);
    const long nq = a.n / 4;
    const long stride = (long)a.nreg * 256;
    // the workgroup's 256 quads of an iteration start at ib (uniform): the descriptor ranges they
    // can meet are found with scalar loads, each lane then tests only those (ascending q0)
    int j = 0;
    for (long ib = (long)b * 256; ib < nq; ib += stride) {
      while (j < a.nslab && a.q1[j] <= ib) ++j;
      j = __builtin_amdgcn_readfirstlane(j);
      const long i = ib + tid;
      if (i >= nq) break;
      bool own = true;
      for (int t = j; t < a.nslab && a.q0[t] < ib + 256; ++t) own = own && !(i >= a.q0[t] && i < a.q1[t]);
      if (own) adam_quad<LOWP>(a, k, i, reinterpret_cast<const f32x4*>(a.g)[i]);
    }
    if (b == 0 && tid < a.n - nq * 4) {
      const long i = nq * 4 + tid;
      adam_one<LOWP>(a, k, i, a.g[i]);
    }
    return;
  }
  // the descriptor of this workgroup
  const int sb = (int)blockIdx.x;
  int d = 0;
  while (d + 1 < a.nslab && sb >= a.blk0[d + 1]) ++d;
  d = __builtin_amdgcn_readfirstlane(d);
  const vae_grad_slab& s = a.s[d];
  const int lb = sb - a.blk0[d];
  const long count = s.count, ld = s.ld;
  const int rows = s.rows;
  const long base = a.off[d];
  if (a.tall[d]) {
    __shared__ float red[16][17];
    const int c = tid & 15, part = tid >> 4;
    const long col = (long)lb * 16 + c;
    // the element's optimizer state goes out first: its round trip overlaps the column sums
    const long e = (long)lb * 16 + tid;
    const bool upd = tid < 16 && e < ((count + 15) & ~15L);
    float pi = 0.f, mi = 0.f, vi = 0.f;
    if (upd) { pi = a.p[base + e]; mi = a.m[base + e]; vi = a.v[base + e]; }
    float acc = 0.f;
    if (col < count) {
      int r = part;
      for (; r + 16 * 7 < rows; r += 16 * 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = s.slab[(long)(r + 16 * u) * ld + col];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += t[u];
      }
      for (; r < rows; r += 16) acc += s.slab[(long)r * ld + col];
    }
    red[part][c] = acc;
    __syncthreads();
    if (upd) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) t += red[q][tid];
      // (elements past count up to the 16-column boundary are not the descriptor's: their own
      // gradient)
      const float gv = e < count ? t : a.g[base + e];
      a.g[base + e] = gv;
      adam_elem(k, pi, gv, mi, vi);
      a.m[base + e] = mi; a.v[base + e] = vi; a.p[base + e] = pi;
      if (LOWP) a.lowp[base + e] = (__bf16)pi;
    }
    return;
  }
  // short: one quad per thread, rows in ascending order (the K slices of a grouped weight gradient:
  // 1-32 rows), the quad's optimizer state loaded first so both round trips overlap
  const long q = (long)lb * 256 + tid;
  const long e0 = q * 4;
  if (e0 >= count) return;
  const long gi = (base + e0) / 4;
  f32x4 p4 = reinterpret_cast<const f32x4*>(a.p)[gi];
  f32x4 m4 = reinterpret_cast<const f32x4*>(a.m)[gi];
  f32x4 v4 = reinterpret_cast<const f32x4*>(a.v)[gi];
  const bool vec = (((uintptr_t)s.slab) & 15) == 0 && (ld & 3) == 0;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (vec && e0 + 4 <= count) {
    int r = 0;
    for (; r + 6 <= rows; r += 6) {
      f32x4 t[6];
#pragma unroll
      for (int u = 0; u < 6; ++u) t[u] = *reinterpret_cast<const f32x4*>(s.slab + (long)(r + u) * ld + e0);
#pragma unroll
      for (int u = 0; u < 6; ++u) acc += t[u];
    }
    for (; r < rows; ++r) acc += *reinterpret_cast<const f32x4*>(s.slab + (long)r * ld + e0);
  } else {
    for (int r = 0; r < rows; ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + u < count) acc[u] += s.slab[(long)r * ld + e0 + u];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e0 + u >= count) acc[u] = a.g[base + e0 + u];     // (past the descriptor: its own gradient)
  }
  reinterpret_cast<f32x4*>(a.g)[gi] = acc;
  float pe[4], me[4], ve[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    pe[u] = p4[u]; me[u] = m4[u]; ve[u] = v4[u];
    adam_elem(k, pe[u], acc[u], me[u], ve[u]);
  }
  reinterpret_cast<f32x4*>(a.p)[gi] = f32x4{pe[0], pe[1], pe[2], pe[3]};
  reinterpret_cast<f32x4*>(a.m)[gi] = f32x4{me[0], me[1], me[2], me[3]};
  reinterpret_cast<f32x4*>(a.v)[gi] = f32x4{ve[0], ve[1], ve[2], ve[3]};
  if (LOWP) reinterpret_cast<bf16x4*>(a.lowp)[gi] = bf16x4{(__bf16)pe[0], (__bf16)pe[1], (__bf16)pe[2], (__bf16)pe[3]};
}

}  // namespace

extern "C" int vae_adam_step_ex(const vae_adam_args* a, void* stream) {
  if (!a) return fail(VAE_E_BADARG, "adam_step_ex: args");
  if (a->n <= 0) return VAE_OK;
  if (!a->p || !a->g || !a->m || !a->v || !a->step || !a->lr) return fail(VAE_E_BADARG, "adam_step_ex: null");
  auto al = [](const void* q, uintptr_t n) { return ((uintptr_t)q % n) == 0; };
  if (!al(a->p, 16) || !al(a->g, 16) || !al(a->m, 16) || !al(a->v, 16) || (a->p_lowp && !al(a->p_lowp, 8)))
    return fail(VAE_E_BADARG, "adam_step_ex: buffers must be 16-byte aligned (bf16 copy 8)");
  if (a->nslab < 0 || a->nslab > VAE_SLAB_MAX) return fail(VAE_E_BADARG, "adam_step_ex: %d slabs", a->nslab);
  if (a->has_elbo && (a->elbo.batch <= 0 || a->elbo.batch > 1024 || !a->elbo.out || !a->elbo.sse))
    return fail(VAE_E_BADSHAPE, "adam_step_ex: deferred loss");
  AdamEx k;
  memset(&k, 0, sizeof(k));
  k.n = a->n; k.p = a->p; k.g = a->g; k.m = a->m; k.v = a->v; k.step = a->step; k.lr = a->lr;
  k.b1 = a->beta1; k.b2 = a->beta2; k.eps = a->eps; k.wd = a->weight_decay;
  k.lowp = static_cast<__bf16*>(a->p_lowp);
  // descriptors sorted by their position in g; each must start on a quad and not overlap the next
  // (rows == 0: a gradient its call wrote whole — a plain gradient here)
  int order[VAE_SLAB_MAX], ns = 0;
  for (int i = 0; i < a->nslab; ++i)
    if (a->slab[i].rows != 0) order[ns++] = i;
  std::sort(order, order + ns, [&](int x, int y) { return a->slab[x].dst < a->slab[y].dst; });
  int blk = 0;
  for (int j = 0; j < ns; ++j) {
    const vae_grad_slab& s = a->slab[order[j]];
    const long off = (long)(s.dst - a->g);
    if (!s.dst || !s.slab || s.count <= 0 || s.rows <= 0 || s.ld < s.count || off < 0 || off + s.count > a->n || off % 4)
      return fail(VAE_E_BADARG, "adam_step_ex: slab %d (offset %ld, count %ld)", order[j], off, (long)s.count);
    k.s[j] = s;
    k.off[j] = off;
    k.tall[j] = s.rows >= kTallRows;
    const long span = k.tall[j] ? ((s.count + 15) & ~15L) : ((s.count + 3) & ~3L);
    if (off + span > a->n) return fail(VAE_E_BADARG, "adam_step_ex: slab %d runs past the buffer", order[j]);
    k.q0[j] = off / 4;
    k.q1[j] = (off + span + 3) / 4;
    if (j > 0 && k.q0[j] < k.q1[j - 1]) return fail(VAE_E_BADARG, "adam_step_ex: slabs %d and %d overlap", order[j - 1], order[j]);
    k.blk0[j] = blk;
    blk += (int)(k.tall[j] ? (s.count + 15) / 16 : (s.count + 1023) / 1024);
  }
  k.nslab = ns;
  k.blk0[ns] = blk;
  k.nreg = grid_for((a->n + 3) / 4);
  k.has_elbo = a->has_elbo;
  if (a->has_elbo) k.e = a->elbo;
  const dim3 grid((unsigned)(k.nreg + blk + (a->has_elbo ? 1 : 0)));
  const hipStream_t st = (hipStream_t)stream;
  if (a->p_lowp) VAE_LAUNCH(adam_ex_kernel<true>, grid, dim3(256), 0, st, k);
  else VAE_LAUNCH(adam_ex_kernel<false>, grid, dim3(256), 0, st, k);
  return check_launch("adam_step_ex");
}

extern "C" int vae_cast_bf16(int64_t n, const float* src, void* dst, void* stream) {
  if (n <= 0) return VAE_OK;
  if (!src || !dst) return fail(VAE_E_BADARG, "cast_bf16: null");
  VAE_LAUNCH(cast_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (long)n, src, (__bf16*)dst);
  return check_launch("cast_bf16");
}
