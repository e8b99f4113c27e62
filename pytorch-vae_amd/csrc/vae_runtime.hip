// What every other unit of libvaehip.so links against, and the ABI's housekeeping: the error state
// (fail / check_launch / vae_last_error), vae_abi_version, the launch log, the probe hooks of the
// diagnostics build, the deferred-reduction list, the workspace-size queries, and the ordered
// reduction of the deterministic mode (ordered_sum_launch), which every GEMM launcher calls.
#include <cxxabi.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "vae_common.hpp"

namespace vae {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  if (querying()) return VAE_OK;            // nothing was launched (workspace query)
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail((int)e, "%s: %s", what, hipGetErrorString(e));
  return VAE_OK;
}

namespace {

// The ordered pass of a deterministic call (OrdSum, vae_common.hpp): 32 outputs per workgroup,
// 8 row lanes each taking the rows r = lane (mod 8) in ascending order, the 8 lane totals added
// in lane order — a fixed summation tree whatever the timing.
__global__ void __launch_bounds__(256) ordered_sum_kernel(const OrdSum o) {
  __shared__ float part[8][33];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const long e = (long)blockIdx.x * 32 + cl;
  const bool ok = e < (long)o.groups * o.cols;
  const int g = ok ? (int)(e / o.cols) : 0;
  const int c = ok ? (int)(e - (long)g * o.cols) : 0;
  const int half = c / o.cw, cc = c - half * o.cw;
  const float* base = o.slab + (long)g * o.rpg * o.rstride + (long)half * o.hstride + cc;
  float s = 0.f;
  if (ok) {
    int r = rl;
    for (; r + 24 < o.rpg; r += 32) {                      // 4 rows' loads in flight
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float t = 0.f;
        for (int f = 0; f < o.folds; ++f) t += base[(long)(r + 8 * u) * o.rstride + (long)f * o.fstride];
        v[u] = t;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) s += v[u];
    }
    for (; r < o.rpg; r += 8) {
      float t = 0.f;
      for (int f = 0; f < o.folds; ++f) t += base[(long)r * o.rstride + (long)f * o.fstride];
      s += t;
    }
  }
  part[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && ok) {
    float t = 0.f;
#pragma unroll
    for (int l = 0; l < 8; ++l) t += part[l][cl];
    float* d = o.dst[half] + (long)g * o.gstride + cc;
    *d += t;
  }
}

}  // namespace

int ordered_sum_launch(const OrdSum& o, hipStream_t st) {
  const long outs = (long)o.groups * o.cols;
  if (outs <= 0 || o.rpg <= 0) return VAE_OK;
  if (!o.slab || !o.dst[0] || (o.cols > o.cw && !o.dst[1]))
    return fail(VAE_E_BADARG, "ordered_sum: null slab or destination");
  VAE_LAUNCH(ordered_sum_kernel, dim3((unsigned)((outs + 31) / 32)), dim3(256), 0, st, o);
  return check_launch("ordered_sum");
}
}  // namespace vae

using namespace vae;

extern "C" int vae_abi_version(void) { return VAE_ABI_VERSION; }

extern "C" int vae_launch_log(int32_t on) {
  LaunchLog& l = launch_log();
  if (on) l.n = 0;
  l.on = on ? 1 : 0;
  return VAE_OK;
}

extern "C" int64_t vae_launch_log_names(char* buf, int64_t cap) {
  const LaunchLog& l = launch_log();
  int64_t need = 0;
  for (int i = 0; i < l.n; ++i) {
    const char* m = hipKernelNameRefByPtr(l.k[i], nullptr);
    if (!m) m = "?";
    int st = 0;
    char* d = abi::__cxa_demangle(m, nullptr, nullptr, &st);
    const int w = snprintf(buf && need < cap ? buf + need : nullptr, buf && need < cap ? (size_t)(cap - need) : 0,
                           "%s\t%s\t%d\n", m, (st == 0 && d) ? d : m, l.count[i]);
    free(d);
    need += w > 0 ? w : 0;
  }
  if (buf && cap > 0 && need >= cap) buf[cap - 1] = '\0';
  return need + 1;
}
extern "C" const char* vae_last_error(void) { return g_err; }

#ifdef VAE_PROBE
// Diagnostics build only: device buffer the GEMM kernels append per-block phase records to.
static unsigned long long* g_probe = nullptr;
extern "C" void vae_probe_set(void* buf) { g_probe = static_cast<unsigned long long*>(buf); }
extern "C" unsigned long long* vae_probe_buffer(void) { return g_probe; }
#endif

// ---------------------------------------------------------------------------- deferred reductions
extern "C" int vae_deferred_reset(void) {
  deferred().n = 0;
  deferred().has_elbo = 0;
  return VAE_OK;
}

extern "C" int32_t vae_deferred_take(vae_grad_slab* out, int32_t max, vae_elbo_args* elbo, int32_t* has_elbo) {
  Deferred& d = deferred();
  const int n = d.n;
  for (int i = 0; i < n && i < max && out; ++i) out[i] = d.s[i];
  if (has_elbo) *has_elbo = d.has_elbo;
  if (elbo && d.has_elbo) *elbo = d.elbo;
  d.n = 0;
  d.has_elbo = 0;
  return n;
}

// ---------------------------------------------------------------- workspace queries
// The entry point runs on a copy of the arguments with an unbounded (never dereferenced)
// workspace while the thread's query flag is set: its planning is the real one, every workspace
// site records its bytes (vae_common.hpp ws_fits) and nothing is launched, so the query needs no
// device and no stream.
namespace {
template <class A, class F>
int ws_size(const A* a, size_t* bytes, F&& call) {
  if (!a || !bytes) return fail(VAE_E_BADARG, "workspace_size: null argument");
  A c = *a;
  c.workspace = reinterpret_cast<void*>(uintptr_t(1) << 40);
  c.workspace_bytes = int64_t(1) << 50;
  WsQuery& q = ws_query();
  q.on = 1;
  q.need = 0;
  const int rc = call(&c);
  *bytes = rc ? 0 : (size_t)q.need;
  q.on = 0;
  q.need = 0;
  return rc;
}
}  // namespace

extern "C" int vae_conv2d_workspace_size(const vae_conv_args* a, int32_t op, size_t* bytes) {
  switch (op) {
    case VAE_OP_FWD: return ws_size(a, bytes, [](const vae_conv_args* c) { return vae_conv2d_fwd(c, nullptr); });
    case VAE_OP_BWD_DATA: return ws_size(a, bytes, [](const vae_conv_args* c) { return vae_conv2d_bwd_data(c, nullptr); });
    case VAE_OP_BWD_FILTER: return ws_size(a, bytes, [](const vae_conv_args* c) { return vae_conv2d_bwd_filter(c, nullptr); });
  }
  return fail(VAE_E_BADARG, "conv2d_workspace_size: op %d", op);
}

extern "C" int vae_convT2d_workspace_size(const vae_conv_args* a, int32_t op, size_t* bytes) {
  switch (op) {
    case VAE_OP_FWD: return ws_size(a, bytes, [](const vae_conv_args* c) { return vae_convT2d_fwd(c, nullptr); });
    case VAE_OP_BWD_DATA: return ws_size(a, bytes, [](const vae_conv_args* c) { return vae_convT2d_bwd_data(c, nullptr); });
    case VAE_OP_BWD_FILTER: return ws_size(a, bytes, [](const vae_conv_args* c) { return vae_convT2d_bwd_filter(c, nullptr); });
    case VAE_OP_BWD: return ws_size(a, bytes, [](const vae_conv_args* c) { return vae_convT2d_bwd(c, nullptr); });
  }
  return fail(VAE_E_BADARG, "convT2d_workspace_size: op %d", op);
}

extern "C" int vae_linear_workspace_size(const vae_linear_args* a, int32_t op, size_t* bytes) {
  switch (op) {
    case VAE_OP_FWD: return ws_size(a, bytes, [](const vae_linear_args* c) { return vae_linear_fwd(c, nullptr); });
    case VAE_OP_BWD_DATA: return ws_size(a, bytes, [](const vae_linear_args* c) { return vae_linear_bwd_data(c, nullptr); });
    case VAE_OP_BWD_FILTER: return ws_size(a, bytes, [](const vae_linear_args* c) { return vae_linear_bwd_filter(c, nullptr); });
  }
  return fail(VAE_E_BADARG, "linear_workspace_size: op %d", op);
}

extern "C" int vae_head_workspace_size(const vae_head_args* a, int32_t op, size_t* bytes) {
  switch (op) {
    case VAE_OP_FWD: return ws_size(a, bytes, [](const vae_head_args* c) { return vae_head_fwd(c, nullptr); });
    case VAE_OP_BWD_DATA: return ws_size(a, bytes, [](const vae_head_args* c) { return vae_head_bwd_data(c, nullptr); });
    case VAE_OP_BWD_FILTER: return ws_size(a, bytes, [](const vae_head_args* c) { return vae_head_bwd_filter(c, nullptr); });
    case VAE_OP_BWD: return ws_size(a, bytes, [](const vae_head_args* c) { return vae_head_bwd(c, nullptr); });
  }
  return fail(VAE_E_BADARG, "head_workspace_size: op %d", op);
}
