// multi_device.inc -- one context over several devices (phy_create_multi).
//
// SURVEY.md 8(b)/(e): sites shard naturally.  The reference's boundary is a
// synchronous C++ function called from Stan's log_prob
// (eigen/prune_stan.hpp:9-17); a consumer of that boundary holds ONE handle
// and one host thread.  So the multi-device form lives inside the context:
//   * n shards, shard k a contiguous range of whole 128-pattern blocks
//     (counts differ by <= 1; the last shard takes the ragged tail), each a
//     complete single-device context (phy_create) on devices[k] -- topology
//     and P-matrices redundant, tips / scratch / class plans per shard;
//   * one evaluation = every shard evaluates its patterns on its own stream,
//     then ONE reduction of the fp64 output rows (log L and every gradient
//     are sums over patterns; the Q-parameter chain rule is linear in dL/dP
//     and the root term, so shard rows add up to the whole's):
//       - distinct devices: ncclAllReduce(sum) of the rows, in place, one
//         group call over the shards' communicators (ncclCommInitAll), over
//         xGMI; RCCL is dlopen'ed on first use, so the engine does not
//         depend on it otherwise;
//       - every shard on one device (the one-GPU test box): a device-side
//         sum of the shards' rows in shard order (shard_sum_kernel);
//   * per-site log-likelihoods stay per shard and are gathered into the
//     caller's [n][P] only when asked for.
#include <dlfcn.h>

#include <rccl/rccl.h>

namespace {

constexpr int MAX_SHARDS = 16;

struct RcclApi {
  ncclResult_t (*initAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*allReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                            hipStream_t) = nullptr;
  ncclResult_t (*groupStart)() = nullptr;
  ncclResult_t (*groupEnd)() = nullptr;
  ncclResult_t (*destroy)(ncclComm_t) = nullptr;
  const char* (*errStr)(ncclResult_t) = nullptr;
};

int rccl_api(const RcclApi** out) {
  static RcclApi api;
  static int state = 0;  // 0 untried, 1 ok, -1 unavailable
  if (state == 0) {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (h) {
      api.initAll = reinterpret_cast<decltype(api.initAll)>(dlsym(h, "ncclCommInitAll"));
      api.allReduce = reinterpret_cast<decltype(api.allReduce)>(dlsym(h, "ncclAllReduce"));
      api.groupStart = reinterpret_cast<decltype(api.groupStart)>(dlsym(h, "ncclGroupStart"));
      api.groupEnd = reinterpret_cast<decltype(api.groupEnd)>(dlsym(h, "ncclGroupEnd"));
      api.destroy = reinterpret_cast<decltype(api.destroy)>(dlsym(h, "ncclCommDestroy"));
      api.errStr = reinterpret_cast<decltype(api.errStr)>(dlsym(h, "ncclGetErrorString"));
    }
    state = (api.initAll && api.allReduce && api.groupStart && api.groupEnd && api.destroy && api.errStr) ? 1 : -1;
  }
  if (state < 0) return fail(PHY_EHIP, "RCCL (librccl.so) is not available for a multi-device context");
  *out = &api;
  return PHY_OK;
}

#define NCCL_TRY(api, expr)                                                                    \
  do {                                                                                         \
    ncclResult_t r_ = (expr);                                                                  \
    if (r_ != ncclSuccess) return fail(PHY_EHIP, std::string(#expr) + ": " + (api)->errStr(r_)); \
  } while (0)

struct ShardSum {
  const double* src[MAX_SHARDS];
  int n;
  long long count;
  double* dst;
};

// dst[i] = ((src0[i] + src1[i]) + src2[i]) + ...  (shard order: deterministic)
__global__ void __launch_bounds__(256) shard_sum_kernel(ShardSum a) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.count;
       i += (long long)gridDim.x * blockDim.x) {
    double s = a.src[0][i];
    for (int k = 1; k < a.n; ++k) s += a.src[k][i];
    a.dst[i] = s;
  }
}

struct MultiState {
  std::vector<phy_ctx*> shard;
  std::vector<int> p0, p1;  // pattern range of shard k
  std::vector<hipEvent_t> ev;
  std::vector<ncclComm_t> comm;
  const RcclApi* rccl = nullptr;
  bool same_device = true;
  int P = 0, pending = 0;
};

void free_multi(MultiState* m) {
  if (!m) return;
  for (size_t k = 0; k < m->ev.size(); ++k) {
    (void)hipSetDevice(m->shard[k]->device);
    (void)hipEventDestroy(m->ev[k]);
  }
  if (m->rccl)
    for (ncclComm_t c : m->comm) (void)m->rccl->destroy(c);
  for (phy_ctx* s : m->shard) phy_destroy(s);
  delete m;
}

// Sum the shards' first `count` doubles of d_out into dst (shard 0's
// buffer, or the caller's on shard 0's device), on shard 0's stream `st0`.
int multi_reduce(MultiState* m, long long count, double* dst, hipStream_t st0) {
  const int n = (int)m->shard.size();
  if (m->same_device) {
    HIP_TRY(hipSetDevice(m->shard[0]->device));
    for (int k = 1; k < n; ++k) {
      HIP_TRY(hipEventRecord(m->ev[k], m->shard[k]->stream));
      HIP_TRY(hipStreamWaitEvent(st0, m->ev[k], 0));
    }
    ShardSum ss{};
    for (int k = 0; k < n; ++k) ss.src[k] = (k == 0) ? dst : m->shard[k]->d_out;
    ss.n = n;
    ss.count = count;
    ss.dst = dst;
    const int blocks = (int)std::min<long long>(1024, (count + 255) / 256);
    hipLaunchKernelGGL(shard_sum_kernel, dim3(std::max(1, blocks)), dim3(256), 0, st0, ss);
    HIP_TRY(hipGetLastError());
    // the shards' next evaluation (which rewrites their rows) waits for this sum
    HIP_TRY(hipEventRecord(m->ev[0], st0));
    for (int k = 1; k < n; ++k) HIP_TRY(hipStreamWaitEvent(m->shard[k]->stream, m->ev[0], 0));
    return PHY_OK;
  }
  NCCL_TRY(m->rccl, m->rccl->groupStart());
  for (int k = 0; k < n; ++k) {
    double* buf = (k == 0) ? dst : m->shard[k]->d_out;
    hipStream_t st = (k == 0) ? st0 : m->shard[k]->stream;
    NCCL_TRY(m->rccl, m->rccl->allReduce(buf, buf, (size_t)count, ncclDouble, ncclSum, m->comm[k], st));
  }
  NCCL_TRY(m->rccl, m->rccl->groupEnd());
  return PHY_OK;
}

// Queue a host-buffer evaluation on every shard and the reduction into
// shard 0's d_out (site log-likelihoods into each shard's d_site).
// The caller's buffers are only read during the call: up to PIN_DRAWS draws
// they are copied into shard 0's pinned staging first (the uploads of every
// shard read that copy, so phy_eval_submit may return before they run);
// larger batches are uploaded synchronously.
int multi_enqueue(phy_ctx* ctx, int n, const double* blens, const double* model, bool want_site) {
  MultiState* m = ctx->ms;
  const int ml = 10 + 2 * ctx->pb.C;
  const size_t nb = (size_t)n * ctx->pb.B, nm = (size_t)n * ml;
  const bool staged = n <= PIN_DRAWS && m->shard[0]->h_in;
  if (staged) {
    double* h = m->shard[0]->h_in;
    std::memcpy(h, blens, sizeof(double) * nb);
    std::memcpy(h + nb, model, sizeof(double) * nm);
    blens = h;
    model = h + nb;
  }
  for (phy_ctx* s : m->shard) {
    HIP_TRY(hipSetDevice(s->device));
    if (staged) {
      HIP_TRY(hipMemcpyAsync(s->d_blens, blens, sizeof(double) * nb, hipMemcpyHostToDevice, s->stream));
      HIP_TRY(hipMemcpyAsync(s->d_model, model, sizeof(double) * nm, hipMemcpyHostToDevice, s->stream));
    } else {
      HIP_TRY(hipStreamSynchronize(s->stream));
      HIP_TRY(hipMemcpy(s->d_blens, blens, sizeof(double) * nb, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(s->d_model, model, sizeof(double) * nm, hipMemcpyHostToDevice));
    }
    int rc = launch(s, n, s->d_blens, s->d_model, s->d_out, want_site ? s->d_site : nullptr, s->stream);
    if (rc) return rc;
  }
  phy_ctx* s0 = m->shard[0];
  return multi_reduce(m, (long long)n * phy_output_len(s0), s0->d_out, s0->stream);
}

// Rows (shard 0's reduced d_out) and site log-likelihoods to the host; waits.
int multi_collect(phy_ctx* ctx, int n, double* out, double* site_ll) {
  MultiState* m = ctx->ms;
  phy_ctx* s0 = m->shard[0];
  HIP_TRY(hipSetDevice(s0->device));
  HIP_TRY(hipMemcpyAsync(out, s0->d_out, sizeof(double) * n * phy_output_len(s0), hipMemcpyDeviceToHost, s0->stream));
  if (site_ll)
    for (size_t k = 0; k < m->shard.size(); ++k) {
      phy_ctx* s = m->shard[k];
      const int pk = m->p1[k] - m->p0[k];
      HIP_TRY(hipSetDevice(s->device));
      HIP_TRY(hipMemcpy2DAsync(site_ll + m->p0[k], sizeof(double) * m->P, s->d_site, sizeof(double) * pk,
                               sizeof(double) * pk, n, hipMemcpyDeviceToHost, s->stream));
    }
  for (phy_ctx* s : m->shard) {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return PHY_OK;
}

int multi_eval(phy_ctx* ctx, int n, const double* blens, const double* model, double* out, double* site_ll) {
  if (ctx->ms->pending) return fail(PHY_EINVAL, "phy_eval: a phy_eval_submit is still in flight (phy_eval_wait first)");
  if (n < 1 || n > ctx->pb.max_draws) return fail(PHY_ERANGE, "n_draws out of range");
  if (!blens || !model || !out) return fail(PHY_EINVAL, "NULL host buffer");
  int rc = multi_enqueue(ctx, n, blens, model, site_ll != nullptr);
  if (rc) return rc;
  return multi_collect(ctx, n, out, site_ll);
}

// Device buffers on shard 0's device: shard 0 evaluates into d_out, the
// others take peer copies of the inputs, then the reduction into d_out.
int multi_eval_device(phy_ctx* ctx, int n, const double* d_blens, const double* d_model, double* d_out,
                      double* d_site, void* stream) {
  MultiState* m = ctx->ms;
  if (m->pending) return fail(PHY_EINVAL, "phy_eval_device: a phy_eval_submit is still in flight");
  if (n < 1 || n > ctx->pb.max_draws) return fail(PHY_ERANGE, "n_draws out of range");
  if (!d_blens || !d_model || !d_out) return fail(PHY_EINVAL, "NULL device buffer");
  if (d_site) return fail(PHY_EINVAL, "phy_eval_device on a multi-device context: per-site log-likelihoods "
                                      "are gathered by phy_eval only");
  phy_ctx* s0 = m->shard[0];
  HIP_TRY(hipSetDevice(s0->device));
  if (!stream)  // the caller's legacy null stream: shard 0's stream, fenced both ways (phy_eval_device)
    return null_fenced(s0, [&](hipStream_t st) { return multi_eval_device(ctx, n, d_blens, d_model, d_out, d_site, st); });
  hipStream_t st0 = reinterpret_cast<hipStream_t>(stream);
  const int ml = 10 + 2 * ctx->pb.C;
  HIP_TRY(hipEventRecord(m->ev[0], st0));  // the inputs are ready on the caller's stream
  for (size_t k = 1; k < m->shard.size(); ++k) {
    phy_ctx* s = m->shard[k];
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamWaitEvent(s->stream, m->ev[0], 0));
    HIP_TRY(hipMemcpyPeerAsync(s->d_blens, s->device, d_blens, s0->device, sizeof(double) * n * ctx->pb.B, s->stream));
    HIP_TRY(hipMemcpyPeerAsync(s->d_model, s->device, d_model, s0->device, sizeof(double) * n * ml, s->stream));
    int rc = launch(s, n, s->d_blens, s->d_model, s->d_out, nullptr, s->stream);
    if (rc) return rc;
  }
  HIP_TRY(hipSetDevice(s0->device));
  int rc = launch(s0, n, d_blens, d_model, d_out, nullptr, st0);
  if (rc) return rc;
  rc = multi_reduce(m, (long long)n * phy_output_len(s0), d_out, st0);
  if (rc) return rc;
  if (!m->same_device)  // the other shards' buffers are reused by the next call: join their streams
    for (size_t k = 1; k < m->shard.size(); ++k) {
      HIP_TRY(hipSetDevice(m->shard[k]->device));
      HIP_TRY(hipEventRecord(m->ev[k], m->shard[k]->stream));
      HIP_TRY(hipSetDevice(s0->device));
      HIP_TRY(hipStreamWaitEvent(st0, m->ev[k], 0));
    }
  return PHY_OK;
}

}  // namespace
