// api_host.hip -- the host-pointer entry points of include/nflhip.h.  Each one checks its arguments and then runs the matching
// device-pointer entry (api.hip) on staging buffers the context owns: small calls through the context's four staging slots,
// large batches through a three-slot pipeline of pinned chunks.
#include "../../include/nflhip.h"
#include "../../include/nflhip_debug.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"

// Large batches through the host-pointer entry points (what an unchanged caller holding arrays of inline-storage
// nfl::poly gets: poly.hpp:87-88, tests/tools.h:6-17).  hipMemcpy from pageable memory tops out at ~12 GB/s on this
// platform (the runtime's single staging thread), 5x below PCIe.  Here the batch is cut into chunks that flow through
// three slots of PINNED staging buffers: several host threads copy chunk k + 1 into its slot while chunk k crosses PCIe
// (H2D stream), chunk k - 1 is computed (compute stream) and chunk k - 2 returns (D2H stream) and is copied out.
// Results are what one call over the whole batch gives (every operation here is per-polynomial).
namespace {
class CopyPool {  // a few host threads that memcpy slices; process-wide, started on first use
 public:
  static CopyPool &get() {
    static CopyPool *p = new CopyPool();  // (leaked on purpose: worker threads must not be joined from a static destructor)
    return *p;
  }
  void copy(void *dst, const void *src, size_t bytes) {
    const size_t slice = 512 << 10;
    const size_t parts = (bytes + slice - 1) / slice;
    if (parts <= 1 || workers_.empty()) {
      std::memcpy(dst, src, bytes);
      return;
    }
    // ONE job at a time: the pool is process-wide and keeps a single job's state, while callers on different contexts
    // (one host thread per GPU, two ring types) hold only their own context's lock
    std::lock_guard<std::mutex> call(call_mu_);
    std::unique_lock<std::mutex> lk(mu_);
    dst_ = (char *)dst;
    src_ = (const char *)src;
    bytes_ = bytes;
    slice_ = slice;
    next_ = 0;
    parts_ = parts;
    done_ = 0;
    ++generation_;
    gen_hint_.store(generation_, std::memory_order_release);
    cv_.notify_all();
    lk.unlock();
    work();  // the calling thread copies too
    lk.lock();
    cv_done_.wait(lk, [&] { return done_ == parts_; });
  }

 private:
  CopyPool() {
    unsigned n = std::thread::hardware_concurrency();
    n = n >= 64 ? 15 : (n > 16 ? 7 : (n > 2 ? n / 2 - 1 : 0));  // + the caller: 16 copying threads on a server host
    for (unsigned i = 0; i < n; ++i) workers_.emplace_back([this] { loop(); }), workers_.back().detach();
  }
  void work() {
    for (;;) {
      size_t k;
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (next_ >= parts_) return;
        k = next_++;
      }
      const size_t off = k * slice_, len = bytes_ - off < slice_ ? bytes_ - off : slice_;
      std::memcpy(dst_ + off, src_ + off, len);
      std::lock_guard<std::mutex> lk(mu_);
      if (++done_ == parts_) cv_done_.notify_all();
    }
  }
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      // a chunk is ~0.3 ms of copying for one thread: a sleeping worker wakes too late to help, so workers spin for a
      // while after every job (the next chunk follows within microseconds while a call is in flight) and only then sleep
      bool got = false;
      for (int spin = 0; spin < 20000 && !got; ++spin) {
        if (gen_hint_.load(std::memory_order_acquire) != seen) got = true;
        else __builtin_ia32_pause();
      }
      {
        std::unique_lock<std::mutex> lk(mu_);
        if (!got) cv_.wait(lk, [&] { return generation_ != seen; });
        seen = generation_;
      }
      work();
    }
  }
  std::atomic<unsigned long long> gen_hint_{0};
  std::mutex mu_, call_mu_;
  std::condition_variable cv_, cv_done_;
  std::vector<std::thread> workers_;
  char *dst_ = nullptr;
  const char *src_ = nullptr;
  size_t bytes_ = 0, slice_ = 0, next_ = 0, parts_ = 0, done_ = 0;
  unsigned long long generation_ = 0;
};
}  // namespace

struct HostPipe {
  static constexpr int kSlots = 3, kBufs = 4;            // per slot: up to 3 inputs + 1 output
  static constexpr size_t kChunkBytes = size_t(8) << 20;  // per operand and slot
  void *pinned[kSlots][kBufs] = {};
  void *dev[kSlots][kBufs] = {};
  hipStream_t s_h2d = nullptr, s_d2h = nullptr;
  hipEvent_t ev_h2d[kSlots] = {}, ev_k[kSlots] = {}, ev_d2h[kSlots] = {};
  double t_in = 0, t_out = 0, t_wait = 0, t_total = 0;   // seconds spent copying in / out, waiting for the device, in calls
  ~HostPipe() {
    for (int s = 0; s < kSlots; ++s) {
      for (int b = 0; b < kBufs; ++b) {
        if (pinned[s][b]) (void)hipHostFree(pinned[s][b]);
        if (dev[s][b]) (void)hipFree(dev[s][b]);
      }
      if (ev_h2d[s]) (void)hipEventDestroy(ev_h2d[s]);
      if (ev_k[s]) (void)hipEventDestroy(ev_k[s]);
      if (ev_d2h[s]) (void)hipEventDestroy(ev_d2h[s]);
    }
    if (s_h2d) (void)hipStreamDestroy(s_h2d);
    if (s_d2h) (void)hipStreamDestroy(s_d2h);
  }
};

void pipe_destroy(nflhip_ctx *ctx) {
  delete ctx->pipe;
  ctx->pipe = nullptr;
}

static int pipe_get(nflhip_ctx *ctx, HostPipe **out) {
  if (!ctx->pipe) {
    std::unique_ptr<HostPipe> p(new (std::nothrow) HostPipe());
    if (!p) return fail(ctx, NFLHIP_ERR_NOMEM, "out of host memory");
    HIPCHK(ctx, hipStreamCreateWithFlags(&p->s_h2d, hipStreamNonBlocking));
    HIPCHK(ctx, hipStreamCreateWithFlags(&p->s_d2h, hipStreamNonBlocking));
    for (int s = 0; s < HostPipe::kSlots; ++s) {
      for (int b = 0; b < HostPipe::kBufs; ++b) {
        HIPCHK(ctx, hipHostMalloc(&p->pinned[s][b], HostPipe::kChunkBytes, hipHostMallocDefault));
        HIPCHK(ctx, hipMalloc(&p->dev[s][b], HostPipe::kChunkBytes));
      }
      HIPCHK(ctx, hipEventCreateWithFlags(&p->ev_h2d[s], hipEventDisableTiming));
      HIPCHK(ctx, hipEventCreateWithFlags(&p->ev_k[s], hipEventDisableTiming));
      HIPCHK(ctx, hipEventCreateWithFlags(&p->ev_d2h[s], hipEventDisableTiming));
    }
    ctx->pipe = p.release();
  }
  *out = ctx->pipe;
  return NFLHIP_OK;
}

// in[j] (nin <= 3 host arrays of `batch` polynomials) -> out (host array); launch(d_in[], d_out, count, stream) enqueues
// the per-polynomial operation on a chunk.  Caller holds ctx->mu.  Returns NFLHIP_ERR_UNSUPPORTED when the batch is too
// small to pipeline (the simple staged path then serves it).
template <typename F>
static int run_pipelined(nflhip_ctx *ctx, size_t batch, const void *const *in, int nin, void *out, F launch) {
  const size_t pb = poly_bytes(ctx, 1);
  const size_t per = HostPipe::kChunkBytes / pb;  // polynomials per chunk
  if (per == 0 || batch < 2 * per) return NFLHIP_ERR_UNSUPPORTED;
  HostPipe *p = nullptr;
  int rc = pipe_get(ctx, &p);
  if (rc) return rc;
  CopyPool &pool = CopyPool::get();
  const size_t nchunks = (batch + per - 1) / per;
  auto count_of = [&](size_t k) { return k + 1 < nchunks ? per : batch - k * per; };
  typedef std::chrono::steady_clock clk;
  auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  const clk::time_point t_begin = clk::now();
  // chunk k is back in its pinned slot: hand it to the caller.  Done by a SECOND host thread, so that results leave while
  // the calling thread (and the pool) copies the next chunks in: the two directions overlap on the host as they do on PCIe
  std::atomic<size_t> issued{0}, drained{0};
  std::atomic<int> drain_rc{NFLHIP_OK};
  std::atomic<bool> stop{false};
  std::string drain_err;
  auto drain_one = [&](size_t k) -> int {
    const int s = int(k % HostPipe::kSlots);
    const clk::time_point t0 = clk::now();
    hipError_t he = hipEventSynchronize(p->ev_d2h[s]);
    if (he != hipSuccess) {
      drain_err = std::string("hipEventSynchronize: ") + hipGetErrorString(he);
      return NFLHIP_ERR_HIP;
    }
    const clk::time_point t1 = clk::now();
    std::memcpy((char *)out + k * per * pb, p->pinned[s][3], count_of(k) * pb);
    p->t_wait += secs(t0, t1);
    p->t_out += secs(t1, clk::now());
    return NFLHIP_OK;
  };
  std::thread drainer;
  try {
    drainer = std::thread([&] {
      (void)hipSetDevice(ctx->device);
      for (size_t k = 0; k < nchunks; ++k) {
        while (issued.load(std::memory_order_acquire) <= k) {
          if (stop.load(std::memory_order_acquire)) return;
          __builtin_ia32_pause();
        }
        const int r = drain_one(k);
        if (r) { drain_rc.store(r); return; }
        drained.store(k + 1, std::memory_order_release);
      }
    });
  } catch (...) {  // (no exception crosses the C boundary)
    return fail(ctx, NFLHIP_ERR_NOMEM, "cannot start the host thread that copies results out");
  }
  // Whatever way this function is left: the drainer is joined, and -- on an error path, where copies and kernels may still
  // be in flight on the three streams against the pinned and device slots -- the streams are drained before the slots
  // can be reused by the next call on this context
  bool completed = false;
  struct joiner {
    std::thread &t; std::atomic<bool> &stop; bool &completed; HostPipe *p; nflhip_ctx *ctx;
    ~joiner() {
      stop.store(true);
      if (t.joinable()) t.join();
      if (!completed) {
        (void)hipStreamSynchronize(p->s_h2d);
        (void)hipStreamSynchronize(ctx->hstream);
        (void)hipStreamSynchronize(p->s_d2h);
        (void)hipGetLastError();
      }
    }
  } join_guard{drainer, stop, completed, p, ctx};
  for (size_t k = 0; k < nchunks; ++k) {
    const int s = int(k % HostPipe::kSlots);
    while (k >= size_t(HostPipe::kSlots) && drained.load(std::memory_order_acquire) + HostPipe::kSlots <= k) {  // the slot's previous tenant
      if (drain_rc.load()) return fail(ctx, drain_rc.load(), drain_err);
      __builtin_ia32_pause();
    }
    const size_t cnt = count_of(k), bytes = cnt * pb;
    const void *d_in[3] = {nullptr, nullptr, nullptr};
    for (int j = 0; j < nin; ++j) {
      // (aliased operands -- polymul(a, a) -- are staged once)
      int same = -1;
      for (int i = 0; i < j; ++i)
        if (in[i] == in[j]) same = i;
      if (same >= 0) { d_in[j] = d_in[same]; continue; }
      const clk::time_point t0 = clk::now();
      pool.copy(p->pinned[s][j], (const char *)in[j] + k * per * pb, bytes);
      p->t_in += secs(t0, clk::now());
      HIPCHK(ctx, hipMemcpyAsync(p->dev[s][j], p->pinned[s][j], bytes, hipMemcpyHostToDevice, p->s_h2d));
      d_in[j] = p->dev[s][j];
    }
    HIPCHK(ctx, hipEventRecord(p->ev_h2d[s], p->s_h2d));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->hstream, p->ev_h2d[s], 0));
    rc = launch(d_in, p->dev[s][3], cnt, (void *)ctx->hstream);
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(p->ev_k[s], ctx->hstream));
    HIPCHK(ctx, hipStreamWaitEvent(p->s_d2h, p->ev_k[s], 0));
    HIPCHK(ctx, hipMemcpyAsync(p->pinned[s][3], p->dev[s][3], bytes, hipMemcpyDeviceToHost, p->s_d2h));
    HIPCHK(ctx, hipEventRecord(p->ev_d2h[s], p->s_d2h));
    // (the next H2D into this slot's device inputs cannot overtake this chunk's kernel: the host reuses a slot only after
    // its result has been drained.  No wait on the in-order H2D stream here -- it would hold chunk k + 1's copy, which
    // goes to ANOTHER slot, behind kernel k, and copies would never overlap compute)
    issued.store(k + 1, std::memory_order_release);
  }
  while (drained.load(std::memory_order_acquire) < nchunks) {
    if (drain_rc.load()) return fail(ctx, drain_rc.load(), drain_err);
    __builtin_ia32_pause();
  }
  p->t_total += secs(t_begin, clk::now());
  completed = true;
  return NFLHIP_OK;
}

// The simple staged path of one call, under the context's lock.  Every host-pointer call ends with ctx->hstream drained, so
// in() may fill a pinned slot with a plain memcpy.  A call that leaves after its first in() without its result copied out
// (an error on the way) drains the stream here: launches queued before the failing step may still use the slots, which the
// next call refills from the host or frees when it grows them.
namespace {
struct Staged {
  nflhip_ctx *ctx;
  std::unique_lock<std::mutex> lk;
  bool pending = false;  // work of this call may still be in flight on ctx->hstream
  explicit Staged(nflhip_ctx *c) : ctx(c), lk(c->mu) {}
  ~Staged() {
    if (pending) {
      (void)hipStreamSynchronize(ctx->hstream);
      (void)hipGetLastError();
    }
  }
  int in(int slot, const void *h, size_t bytes) {   // (h NULL: the slot is only made large enough)
    pending = true;
    int rc = ensure_stage(ctx, slot, bytes);
    if (rc) return rc;
    if (h && ctx->stage_host[slot]) std::memcpy(ctx->stage[slot], h, bytes);
    else if (h) HIPCHK(ctx, hipMemcpyAsync(ctx->stage[slot], h, bytes, hipMemcpyHostToDevice, ctx->hstream));
    return NFLHIP_OK;
  }
  // `count` results of `bytes` each, one behind the other in the slot
  int outs(void *const *h, size_t count, int slot, size_t bytes) {
    const char *s = (const char *)ctx->stage[slot];
    if (!ctx->stage_host[slot])
      for (size_t k = 0; k < count; ++k) HIPCHK(ctx, hipMemcpyAsync(h[k], s + k * bytes, bytes, hipMemcpyDeviceToHost, ctx->hstream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->hstream));
    pending = false;
    if (ctx->stage_host[slot])
      for (size_t k = 0; k < count; ++k) std::memcpy(h[k], s + k * bytes, bytes);
    return NFLHIP_OK;
  }
  int out(void *h, int slot, size_t bytes) { return outs(&h, 1, slot, bytes); }
  int out2(void *h0, void *h1, int slot, size_t bytes) {
    void *const h[2] = {h0, h1};
    return outs(h, 2, slot, bytes);
  }
};

// An operand of a staged call: `bytes` of host memory at h, staged into slot `slot`.  h NULL: an operand the call does not
// read -- nothing is staged, the device call gets the slot's buffer as it is (the pipeline: operand 0's chunk).
struct HostIn { int slot; const void *h; size_t bytes; };
// Its result: `bytes` copied from slot `slot` to h.  slot < 0: the device call hands its result back itself, having drained
// the stream.
struct HostOut { int slot; void *h; size_t bytes; };
}  // namespace

// Every host-pointer entry that computes on the device runs here once its arguments are checked.  With `pipelined` a batch
// large enough takes the pinned pipeline; otherwise the inputs are staged in order, the result slot is made large enough,
// and op(in[], out, batch, stream) runs once on the slots' buffers before the result is copied out.  op is the pipeline's
// per-chunk launch as well (in[] the chunk's inputs, out its result buffer).
template <typename Op>
static int staged_call(nflhip_ctx *ctx, size_t batch, bool pipelined, const HostIn *ins, int nin, HostOut res, Op op) {
  Staged s(ctx);
  const void *d[4] = {nullptr, nullptr, nullptr, nullptr};
  if (pipelined) {
    for (int j = 0; j < nin; ++j) d[j] = ins[j].h ? ins[j].h : ins[0].h;
    const int rc = run_pipelined(ctx, batch, d, nin, res.h, op);
    if (rc != NFLHIP_ERR_UNSUPPORTED) return rc;
  }
  for (int j = 0; j < nin; ++j) {
    const int rc = ins[j].h ? s.in(ins[j].slot, ins[j].h, ins[j].bytes) : NFLHIP_OK;
    if (rc) return rc;
  }
  const int rc = res.slot >= 0 ? s.in(res.slot, nullptr, res.bytes) : NFLHIP_OK;
  if (rc) return rc;
  for (int j = 0; j < nin; ++j) d[j] = ctx->stage[ins[j].slot];
  const int orc = op(d, res.slot >= 0 ? ctx->stage[res.slot] : nullptr, batch, (void *)ctx->hstream);
  if (orc) return orc;
  if (res.slot >= 0) return s.out(res.h, res.slot, res.bytes);
  s.pending = false;
  return NFLHIP_OK;
}

extern "C" {

void nflhip_debug_host_pipe_seconds(const nflhip_ctx *ctx, double out[4]) {
  const HostPipe *p = ctx ? ctx->pipe : nullptr;
  out[0] = p ? p->t_in : 0;
  out[1] = p ? p->t_out : 0;
  out[2] = p ? p->t_wait : 0;
  out[3] = p ? p->t_total : 0;
}

// the transforms run in place: a pipeline chunk is first copied into its result buffer
static int ntt_host(nflhip_ctx *ctx, void *h, size_t batch, int (*dev)(nflhip_ctx *, void *, size_t, void *)) {
  CHECK_CTX(ctx);
  if (batch == 0) return NFLHIP_OK;
  if (!h) return fail(ctx, NFLHIP_ERR_INVALID, "NULL data pointer");
  const size_t bytes = poly_bytes(ctx, batch);
  const HostIn ins[] = {{0, h, bytes}};
  return staged_call(ctx, batch, true, ins, 1, {0, h, bytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    if (o != d[0]) HIPCHK(ctx, hipMemcpyAsync(o, d[0], poly_bytes(ctx, cnt), hipMemcpyDeviceToDevice, (hipStream_t)st));
    return dev(ctx, o, cnt, st);
  });
}
int nflhip_ntt_fwd(nflhip_ctx *ctx, void *h, size_t batch) { return ntt_host(ctx, h, batch, nflhip_ntt_fwd_dev); }
int nflhip_ntt_inv(nflhip_ctx *ctx, void *h, size_t batch) { return ntt_host(ctx, h, batch, nflhip_ntt_inv_dev); }

int nflhip_automorphism(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, uint64_t k, int form) {
  CHECK_CTX(ctx);
  if (form != NFLHIP_FORM_COEFF && form != NFLHIP_FORM_NTT) return fail(ctx, NFLHIP_ERR_INVALID, "unknown polynomial form");
  if ((k & 1) == 0) return fail(ctx, NFLHIP_ERR_INVALID, "automorphism exponent k must be odd");
  if (batch == 0) return NFLHIP_OK;
  if (!h_out || !h_in) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t bytes = poly_bytes(ctx, batch);
  if (h_out != h_in && bytes_overlap(h_out, h_in, bytes)) return fail(ctx, NFLHIP_ERR_INVALID, "the output overlaps the input");
  const HostIn ins[] = {{0, h_in, bytes}};
  return staged_call(ctx, batch, true, ins, 1, {1, h_out, bytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    return nflhip_automorphism_dev(ctx, o, d[0], cnt, k, form, st);
  });
}

// RNS rescale: the result is one row per polynomial shorter than the input, so the call is staged whole (the pipeline's chunks
// assume operands of one size)
int nflhip_rescale(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, int form) {
  int rc = rescale_check(ctx, h_out, h_in, batch, form, true);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t bytes = poly_bytes(ctx, batch), obytes = bytes - batch * ctx->shape.n * ctx->word;
  const HostIn ins[] = {{0, h_in, bytes}};
  return staged_call(ctx, batch, false, ins, 1, {1, h_out, obytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    return nflhip_rescale_dev(ctx, o, d[0], cnt, form, st);
  });
}

// RNS base conversion: rows D of the output, every other row as the input has it (staged whole: the result buffer starts as a copy
// of the input); mod-down: the result is k rows per polynomial shorter than the input
int nflhip_baseconv(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags) {
  int rc = baseconv_check(ctx, h_out, h_in, batch, s0, ks, d0, kd, flags, false);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t bytes = poly_bytes(ctx, batch);
  const HostIn ins[] = {{0, h_in, bytes}};
  return staged_call(ctx, batch, false, ins, 1, {1, h_out, bytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    // (a staging buffer is device memory or pinned host memory: the copy kind is left to the runtime)
    if (o != d[0]) HIPCHK(ctx, hipMemcpyAsync(o, d[0], poly_bytes(ctx, cnt), hipMemcpyDefault, (hipStream_t)st));
    return nflhip_baseconv_dev(ctx, o, o, cnt, s0, ks, d0, kd, flags, st);
  });
}
int nflhip_moddown(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t k, int flags) {
  const size_t nm = ctx ? ctx->shape.nm : 0, kept = k < nm ? nm - k : 0;
  int rc = baseconv_check(ctx, h_out, h_in, batch, kept, k, 0, kept, flags, true);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t bytes = poly_bytes(ctx, batch), obytes = batch * kept * ctx->shape.n * ctx->word;
  const HostIn ins[] = {{0, h_in, bytes}};
  return staged_call(ctx, batch, false, ins, 1, {1, h_out, obytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    return nflhip_moddown_dev(ctx, o, d[0], cnt, k, flags, st);
  });
}

// the same on NTT-form data
int nflhip_baseconv_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t s0, size_t ks, size_t d0, size_t kd, int flags) {
  int rc = baseconv_ntt_check(ctx, h_out, h_in, batch, s0, ks, d0, kd, flags, false);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t bytes = poly_bytes(ctx, batch);
  const HostIn ins[] = {{0, h_in, bytes}};
  return staged_call(ctx, batch, false, ins, 1, {1, h_out, bytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    if (o != d[0]) HIPCHK(ctx, hipMemcpyAsync(o, d[0], poly_bytes(ctx, cnt), hipMemcpyDefault, (hipStream_t)st));
    return nflhip_baseconv_ntt_dev(ctx, o, o, cnt, s0, ks, d0, kd, flags, st);
  });
}
int nflhip_moddown_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t k, int flags) {
  const size_t nm = ctx ? ctx->shape.nm : 0, kept = k < nm ? nm - k : 0;
  int rc = baseconv_ntt_check(ctx, h_out, h_in, batch, kept, k, 0, kept, flags, true);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t bytes = poly_bytes(ctx, batch), obytes = batch * kept * ctx->shape.n * ctx->word;
  const HostIn ins[] = {{0, h_in, bytes}};
  return staged_call(ctx, batch, false, ins, 1, {1, h_out, obytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    return nflhip_moddown_ntt_dev(ctx, o, d[0], cnt, k, flags, st);
  });
}

// hybrid key switching: in, the key and both outputs are staged whole (the outputs share one slot, out1 behind out0, so that the
// mod-down runs as one batch).  The body of both entries, the arguments checked: the operands have `level` rows (the top-level entry:
// all nmoduli - k_special, where the level entry on the device forwards), and of the key the digits that are read are staged.
static int keyswitch_host(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_in, const void *h_key, size_t batch, size_t k_special,
                          size_t alpha, size_t level, int flags) {
  int rc = set_device(ctx);
  if (rc) return rc;
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, ob = batch * level * row;
  const size_t kb = 2 * keyswitch_level_digits(ctx, k_special, alpha, level) * nm * row;
  Staged s(ctx);
  if ((rc = s.in(0, h_in, ob)) || (rc = s.in(1, h_key, kb)) || (rc = s.in(2, nullptr, 2 * ob))) return rc;
  char *o = (char *)ctx->stage[2];
  if ((rc = nflhip_keyswitch_level_ntt_dev(ctx, o, o + ob, ctx->stage[0], ctx->stage[1], batch, k_special, alpha, level, flags, (void *)ctx->hstream))) return rc;
  return s.out2(h_out0, h_out1, 2, ob);
}
int nflhip_keyswitch_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_in, const void *h_key, size_t batch, size_t k_special,
                         size_t alpha, int flags) {
  int rc = keyswitch_check(ctx, h_out0, h_out1, h_in, h_key, batch, k_special, alpha, flags);
  if (rc || batch == 0) return rc;
  return keyswitch_host(ctx, h_out0, h_out1, h_in, h_key, batch, k_special, alpha, ctx->shape.nm - k_special, flags);
}
int nflhip_keyswitch_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_in, const void *h_key, size_t batch, size_t k_special,
                               size_t alpha, size_t level, int flags) {
  int rc = level_check(ctx, k_special, level, "keyswitch");
  if (!rc) rc = keyswitch_check(ctx, h_out0, h_out1, h_in, h_key, batch, k_special, alpha, flags, level);
  if (rc || batch == 0) return rc;
  return keyswitch_host(ctx, h_out0, h_out1, h_in, h_key, batch, k_special, alpha, level, flags);
}

// hoisted rotations: c1 (and c0 behind it), every key and every output are staged whole (the outputs share one slot, out0s then out1s).
// The body of both entries, the arguments checked: the operands have `level` rows (the top-level entry: all nmoduli - k_special, where
// the level entry on the device forwards), and of every key the digits that are read are staged.
static int rotate_host(nflhip_ctx *ctx, void *const *h_out0s, void *const *h_out1s, const void *h_c0, const void *h_c1, const void *const *h_keys,
                       const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, size_t level, int flags) {
  int rc = set_device(ctx);
  if (rc) return rc;
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, ob = batch * level * row;
  const size_t kb = 2 * keyswitch_level_digits(ctx, k_special, alpha, level) * nm * row;
  Staged s(ctx);
  if ((rc = s.in(0, nullptr, 2 * ob)) || (rc = s.in(1, nullptr, count * kb)) || (rc = s.in(2, nullptr, 2 * count * ob))) return rc;
  char *c = (char *)ctx->stage[0], *k = (char *)ctx->stage[1], *o = (char *)ctx->stage[2];
  const bool hc = ctx->stage_host[0], hk = ctx->stage_host[1];
  if (hc) std::memcpy(c, h_c1, ob);
  else HIPCHK(ctx, hipMemcpyAsync(c, h_c1, ob, hipMemcpyHostToDevice, ctx->hstream));
  if (h_c0 && hc) std::memcpy(c + ob, h_c0, ob);
  else if (h_c0) HIPCHK(ctx, hipMemcpyAsync(c + ob, h_c0, ob, hipMemcpyHostToDevice, ctx->hstream));
  void *o0[NFLHIP_ROTATE_MAX_OUTPUTS], *o1[NFLHIP_ROTATE_MAX_OUTPUTS];
  const void *keys[NFLHIP_ROTATE_MAX_OUTPUTS];
  for (size_t m = 0; m < count; ++m) {
    if (hk) std::memcpy(k + m * kb, h_keys[m], kb);
    else HIPCHK(ctx, hipMemcpyAsync(k + m * kb, h_keys[m], kb, hipMemcpyHostToDevice, ctx->hstream));
    keys[m] = k + m * kb;
    o0[m] = o + m * ob;
    o1[m] = o + (count + m) * ob;
  }
  if ((rc = nflhip_rotate_hoisted_level_ntt_dev(ctx, o0, o1, h_c0 ? c + ob : nullptr, c, keys, ks, count, batch, k_special, alpha, level, flags,
                                                (void *)ctx->hstream)))
    return rc;
  void *hs[2 * NFLHIP_ROTATE_MAX_OUTPUTS];  // as the slot holds them: out0s, then out1s
  for (size_t m = 0; m < count; ++m) {
    hs[m] = h_out0s[m];
    hs[count + m] = h_out1s[m];
  }
  return s.outs(hs, 2 * count, 2, ob);
}
int nflhip_rotate_hoisted_ntt(nflhip_ctx *ctx, void *const *h_out0s, void *const *h_out1s, const void *h_c0, const void *h_c1,
                              const void *const *h_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, int flags) {
  int rc = rotate_check(ctx, h_out0s, h_out1s, h_c0, h_c1, h_keys, ks, count, batch, k_special, alpha, flags);
  if (rc || batch == 0) return rc;
  return rotate_host(ctx, h_out0s, h_out1s, h_c0, h_c1, h_keys, ks, count, batch, k_special, alpha, ctx->shape.nm - k_special, flags);
}
int nflhip_rotate_hoisted_level_ntt(nflhip_ctx *ctx, void *const *h_out0s, void *const *h_out1s, const void *h_c0, const void *h_c1,
                                    const void *const *h_keys, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                                    size_t level, int flags) {
  int rc = level_check(ctx, k_special, level, "rotate");
  if (!rc) rc = rotate_check(ctx, h_out0s, h_out1s, h_c0, h_c1, h_keys, ks, count, batch, k_special, alpha, flags, level);
  if (rc || batch == 0) return rc;
  return rotate_host(ctx, h_out0s, h_out1s, h_c0, h_c1, h_keys, ks, count, batch, k_special, alpha, level, flags);
}

// weighted sums of automorphisms: every input, every weight and the output (the addend copied into it) are staged whole
int nflhip_automorphism_mac(nflhip_ctx *ctx, void *h_out, const void *h_addend, const void *const *h_ins, const void *const *h_weights,
                            const uint64_t *ks, size_t terms, size_t batch, size_t rows, int flags) {
  int rc = mac_check(ctx, h_out, h_addend, h_ins, h_weights, ks, terms, batch, rows, flags);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t wb = rows * ctx->shape.n * ctx->word, ob = batch * wb;
  Staged s(ctx);
  if ((rc = s.in(0, nullptr, terms * ob)) || (rc = s.in(1, nullptr, terms * wb)) || (rc = s.in(2, h_addend, ob))) return rc;
  char *i = (char *)ctx->stage[0], *w = (char *)ctx->stage[1];
  const void *ins[NFLHIP_MAC_MAX_TERMS], *ws[NFLHIP_MAC_MAX_TERMS];
  for (size_t t = 0; t < terms; ++t) {
    if (ctx->stage_host[0]) std::memcpy(i + t * ob, h_ins[t], ob);
    else HIPCHK(ctx, hipMemcpyAsync(i + t * ob, h_ins[t], ob, hipMemcpyHostToDevice, ctx->hstream));
    if (ctx->stage_host[1]) std::memcpy(w + t * wb, h_weights[t], wb);
    else HIPCHK(ctx, hipMemcpyAsync(w + t * wb, h_weights[t], wb, hipMemcpyHostToDevice, ctx->hstream));
    ins[t] = i + t * ob;
    ws[t] = w + t * wb;
  }
  void *o = ctx->stage[2];
  if ((rc = nflhip_automorphism_mac_dev(ctx, o, h_addend ? o : nullptr, ins, ws, ks, terms, batch, rows, flags, (void *)ctx->hstream))) return rc;
  return s.out(h_out, 2, ob);
}

// slot linear transforms: c1 (and c0 behind it), every key, every weight and both outputs are staged whole (the outputs share one
// slot, out1 behind out0, so that the mod-down runs as one batch).  The body of both entries, as rotate_host; a weight is a whole
// polynomial of this context at every level.
static int lintrans_host(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1, const void *const *h_keys,
                         const void *const *h_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, size_t level,
                         int flags) {
  int rc = set_device(ctx);
  if (rc) return rc;
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, ob = batch * level * row, wb = nm * row;
  const size_t kb = 2 * keyswitch_level_digits(ctx, k_special, alpha, level) * wb;
  Staged s(ctx);
  if ((rc = s.in(0, nullptr, 2 * ob)) || (rc = s.in(1, nullptr, count * (kb + wb))) || (rc = s.in(2, nullptr, 2 * ob))) return rc;
  char *c = (char *)ctx->stage[0], *k = (char *)ctx->stage[1], *o = (char *)ctx->stage[2];
  auto put = [&](int slot, void *d, const void *h, size_t bytes) {
    if (ctx->stage_host[slot]) std::memcpy(d, h, bytes);
    else HIPCHK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->hstream));
    return (int)NFLHIP_OK;
  };
  if ((rc = put(0, c, h_c1, ob)) || (h_c0 && (rc = put(0, c + ob, h_c0, ob)))) return rc;
  const void *keys[NFLHIP_LINTRANS_MAX_TERMS], *ws[NFLHIP_LINTRANS_MAX_TERMS];
  for (size_t m = 0; m < count; ++m) {
    char *km = k + m * (kb + wb);
    if ((h_keys[m] && (rc = put(1, km, h_keys[m], kb))) || (rc = put(1, km + kb, h_weights[m], wb))) return rc;
    keys[m] = h_keys[m] ? km : nullptr;
    ws[m] = km + kb;
  }
  if ((rc = nflhip_lintrans_level_ntt_dev(ctx, o, o + ob, h_c0 ? c + ob : nullptr, c, keys, ws, ks, count, batch, k_special, alpha, level, flags,
                                          (void *)ctx->hstream)))
    return rc;
  return s.out2(h_out0, h_out1, 2, ob);
}
int nflhip_lintrans_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1, const void *const *h_keys,
                        const void *const *h_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha, int flags) {
  int rc = lintrans_check(ctx, h_out0, h_out1, h_c0, h_c1, h_keys, h_weights, ks, count, batch, k_special, alpha, flags);
  if (rc || batch == 0) return rc;
  return lintrans_host(ctx, h_out0, h_out1, h_c0, h_c1, h_keys, h_weights, ks, count, batch, k_special, alpha, ctx->shape.nm - k_special, flags);
}
int nflhip_lintrans_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1, const void *const *h_keys,
                              const void *const *h_weights, const uint64_t *ks, size_t count, size_t batch, size_t k_special, size_t alpha,
                              size_t level, int flags) {
  int rc = level_check(ctx, k_special, level, "lintrans");
  if (!rc) rc = lintrans_check(ctx, h_out0, h_out1, h_c0, h_c1, h_keys, h_weights, ks, count, batch, k_special, alpha, flags, level);
  if (rc || batch == 0) return rc;
  return lintrans_host(ctx, h_out0, h_out1, h_c0, h_c1, h_keys, h_weights, ks, count, batch, k_special, alpha, level, flags);
}

// weighted sums of automorphisms into several outputs: every input, every non-NULL weight and the outputs (an addend copied into its
// output) are staged whole
int nflhip_automorphism_mac_multi(nflhip_ctx *ctx, void *const *h_outs, const void *const *h_addends, const void *const *h_ins,
                                  const void *const *h_weights, const uint64_t *ks, size_t outputs, size_t terms, size_t batch, size_t rows, int flags) {
  int rc = mac_multi_check(ctx, h_outs, h_addends, h_ins, h_weights, ks, outputs, terms, batch, rows, flags);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t wb = rows * ctx->shape.n * ctx->word, ob = batch * wb;
  Staged s(ctx);
  if ((rc = s.in(0, nullptr, terms * ob)) || (rc = s.in(1, nullptr, outputs * terms * wb)) || (rc = s.in(2, nullptr, outputs * ob))) return rc;
  char *i = (char *)ctx->stage[0], *w = (char *)ctx->stage[1], *o = (char *)ctx->stage[2];
  auto put = [&](int slot, void *d, const void *h, size_t bytes) {
    if (ctx->stage_host[slot]) std::memcpy(d, h, bytes);
    else HIPCHK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->hstream));
    return (int)NFLHIP_OK;
  };
  const void *ins[NFLHIP_MAC_MAX_TERMS], *ws[NFLHIP_MAC_MULTI_MAX_OUTPUTS * NFLHIP_MAC_MAX_TERMS], *adds[NFLHIP_MAC_MULTI_MAX_OUTPUTS];
  void *outs[NFLHIP_MAC_MULTI_MAX_OUTPUTS];
  for (size_t t = 0; t < terms; ++t) {
    if ((rc = put(0, i + t * ob, h_ins[t], ob))) return rc;
    ins[t] = i + t * ob;
  }
  for (size_t q = 0; q < outputs * terms; ++q) {
    if (h_weights[q] && (rc = put(1, w + q * wb, h_weights[q], wb))) return rc;
    ws[q] = h_weights[q] ? w + q * wb : nullptr;
  }
  for (size_t q = 0; q < outputs; ++q) {
    const bool add = h_addends && h_addends[q];
    if (add && (rc = put(2, o + q * ob, h_addends[q], ob))) return rc;
    outs[q] = o + q * ob;
    adds[q] = add ? outs[q] : nullptr;
  }
  if ((rc = nflhip_automorphism_mac_multi_dev(ctx, outs, adds, ins, ws, ks, outputs, terms, batch, rows, flags, (void *)ctx->hstream))) return rc;
  return s.outs(h_outs, outputs, 2, ob);
}

// BSGS slot linear transforms: c1 (and c0 behind it), the live digits of every key, every non-NULL weight and both outputs are staged
// whole (the outputs share one slot, out1 behind out0, so that the last mod-down runs as one batch), as lintrans_host
int nflhip_bsgs_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_c0, const void *h_c1, const void *const *h_bkeys, const uint64_t *bks,
                    size_t n1, const void *const *h_gkeys, const uint64_t *gks, size_t n2, const void *const *h_weights, size_t batch, size_t k_special,
                    size_t alpha, size_t level, int flags) {
  int rc = bsgs_check(ctx, h_out0, h_out1, h_c0, h_c1, h_bkeys, bks, n1, h_gkeys, gks, n2, h_weights, batch, k_special, alpha, level, flags);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, ob = batch * level * row, wb = nm * row;
  const size_t kb = 2 * keyswitch_level_digits(ctx, k_special, alpha, level) * wb;
  size_t nk = 0, nw = 0;  // the slot holds what is there: a NULL key or weight takes no room
  for (size_t m = 0; m < n1 + n2; ++m) nk += (m < n1 ? h_bkeys[m] : h_gkeys[m - n1]) != nullptr;
  for (size_t q = 0; q < n1 * n2; ++q) nw += h_weights[q] != nullptr;
  Staged s(ctx);
  if ((rc = s.in(0, nullptr, 2 * ob)) || (rc = s.in(1, nullptr, nk * kb + nw * wb)) || (rc = s.in(2, nullptr, 2 * ob))) return rc;
  char *c = (char *)ctx->stage[0], *k = (char *)ctx->stage[1], *o = (char *)ctx->stage[2], *w = k + nk * kb;
  auto put = [&](int slot, void *d, const void *h, size_t bytes) {
    if (ctx->stage_host[slot]) std::memcpy(d, h, bytes);
    else HIPCHK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->hstream));
    return (int)NFLHIP_OK;
  };
  if ((rc = put(0, c, h_c1, ob)) || (h_c0 && (rc = put(0, c + ob, h_c0, ob)))) return rc;
  const void *keys[NFLHIP_BSGS_MAX_BABY + NFLHIP_BSGS_MAX_GIANT], *ws[NFLHIP_BSGS_MAX_BABY * NFLHIP_BSGS_MAX_GIANT];
  for (size_t m = 0; m < n1 + n2; ++m) {
    const void *h = m < n1 ? h_bkeys[m] : h_gkeys[m - n1];
    keys[m] = nullptr;
    if (!h) continue;
    if ((rc = put(1, k, h, kb))) return rc;
    keys[m] = k;
    k += kb;
  }
  for (size_t q = 0; q < n1 * n2; ++q) {
    ws[q] = nullptr;
    if (!h_weights[q]) continue;
    if ((rc = put(1, w, h_weights[q], wb))) return rc;
    ws[q] = w;
    w += wb;
  }
  if ((rc = nflhip_bsgs_ntt_dev(ctx, o, o + ob, h_c0 ? c + ob : nullptr, c, keys, bks, n1, keys + n1, gks, n2, ws, batch, k_special, alpha, level, flags,
                                (void *)ctx->hstream)))
    return rc;
  return s.out2(h_out0, h_out1, 2, ob);
}

// the tensor product: the inputs share one slot (a0, a1, then b0, b1 unless it is the square), the three outputs another
int nflhip_tensor_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1, const void *h_b0,
                      const void *h_b1, size_t batch, size_t rows, int flags) {
  int rc = tensor_check(ctx, h_out0, h_out1, h_out2, h_a0, h_a1, h_b0, h_b1, batch, rows, flags);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t ob = batch * rows * ctx->shape.n * ctx->word, nin = h_b0 ? 4 : 2;
  Staged s(ctx);
  if ((rc = s.in(0, nullptr, nin * ob)) || (rc = s.in(2, nullptr, 3 * ob))) return rc;
  char *i = (char *)ctx->stage[0], *o = (char *)ctx->stage[2];
  const void *const hin[4] = {h_a0, h_a1, h_b0, h_b1};
  for (size_t k = 0; k < nin; ++k) {
    if (ctx->stage_host[0]) std::memcpy(i + k * ob, hin[k], ob);
    else HIPCHK(ctx, hipMemcpyAsync(i + k * ob, hin[k], ob, hipMemcpyHostToDevice, ctx->hstream));
  }
  if ((rc = nflhip_tensor_ntt_dev(ctx, o, o + ob, o + 2 * ob, i, i + ob, h_b0 ? i + 2 * ob : nullptr, h_b0 ? i + 3 * ob : nullptr, batch, rows, flags,
                                  (void *)ctx->hstream)))
    return rc;
  void *const hout[3] = {h_out0, h_out1, h_out2};
  return s.outs(hout, 3, 2, ob);
}

// scale-and-round by t/Q: the result has fewer rows per polynomial than the input, so the call is staged whole
static int scale_round_host(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t ks, uint64_t t, int flags, bool ntt) {
  size_t obytes = 0;
  int rc = scale_round_check(ctx, h_out, h_in, batch, ks, t, flags, &obytes);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const HostIn ins[] = {{0, h_in, poly_bytes(ctx, batch)}};
  return staged_call(ctx, batch, false, ins, 1, {1, h_out, obytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    return ntt ? nflhip_scale_round_ntt_dev(ctx, o, d[0], cnt, ks, t, flags, st) : nflhip_scale_round_dev(ctx, o, d[0], cnt, ks, t, flags, st);
  });
}
int nflhip_scale_round(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t ks, uint64_t t, int flags) {
  return scale_round_host(ctx, h_out, h_in, batch, ks, t, flags, false);
}
int nflhip_scale_round_ntt(nflhip_ctx *ctx, void *h_out, const void *h_in, size_t batch, size_t ks, uint64_t t, int flags) {
  return scale_round_host(ctx, h_out, h_in, batch, ks, t, flags, true);
}

// the BFV tensor product: staged as the tensor product above
int nflhip_bfv_tensor_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1, const void *h_b0,
                          const void *h_b1, size_t batch, size_t ks, uint64_t t, int flags) {
  int rc = bfv_tensor_check(ctx, h_out0, h_out1, h_out2, h_a0, h_a1, h_b0, h_b1, batch, ks, t, flags);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const size_t ob = batch * ks * ctx->shape.n * ctx->word, nin = h_b0 ? 4 : 2;
  Staged s(ctx);
  if ((rc = s.in(0, nullptr, nin * ob)) || (rc = s.in(2, nullptr, 3 * ob))) return rc;
  char *i = (char *)ctx->stage[0], *o = (char *)ctx->stage[2];
  const void *const hin[4] = {h_a0, h_a1, h_b0, h_b1};
  for (size_t k = 0; k < nin; ++k) {
    if (ctx->stage_host[0]) std::memcpy(i + k * ob, hin[k], ob);
    else HIPCHK(ctx, hipMemcpyAsync(i + k * ob, hin[k], ob, hipMemcpyHostToDevice, ctx->hstream));
  }
  if ((rc = nflhip_bfv_tensor_ntt_dev(ctx, o, o + ob, o + 2 * ob, i, i + ob, h_b0 ? i + 2 * ob : nullptr, h_b0 ? i + 3 * ob : nullptr, batch, ks, t, flags,
                                      (void *)ctx->hstream)))
    return rc;
  void *const hout[3] = {h_out0, h_out1, h_out2};
  return s.outs(hout, 3, 2, ob);
}

// ciphertext multiplication: the inputs (one slot), the key and both outputs are staged whole (the outputs share one slot, out1
// behind out0, so that the mod-down runs as one batch).  The body of both entries, the arguments checked: the operands have `level`
// rows (the top-level entry: all nmoduli - k_special, where the level entry on the device forwards), and of the key the digits that
// are read are staged.
static int mulrelin_host(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1,
                         const void *h_key, size_t batch, size_t k_special, size_t alpha, size_t level, int flags) {
  int rc = set_device(ctx);
  if (rc) return rc;
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, ib = batch * level * row;
  const size_t ob = (flags & NFLHIP_MULRELIN_RESCALE) ? ib - batch * row : ib, nin = h_b0 ? 4 : 2;
  const size_t kb = 2 * keyswitch_level_digits(ctx, k_special, alpha, level) * nm * row;
  Staged s(ctx);
  if ((rc = s.in(0, nullptr, nin * ib)) || (rc = s.in(1, h_key, kb)) || (rc = s.in(2, nullptr, 2 * ob))) return rc;
  char *i = (char *)ctx->stage[0], *o = (char *)ctx->stage[2];
  const void *const hin[4] = {h_a0, h_a1, h_b0, h_b1};
  for (size_t k = 0; k < nin; ++k) {
    if (ctx->stage_host[0]) std::memcpy(i + k * ib, hin[k], ib);
    else HIPCHK(ctx, hipMemcpyAsync(i + k * ib, hin[k], ib, hipMemcpyHostToDevice, ctx->hstream));
  }
  if ((rc = nflhip_mulrelin_level_ntt_dev(ctx, o, o + ob, i, i + ib, h_b0 ? i + 2 * ib : nullptr, h_b0 ? i + 3 * ib : nullptr, ctx->stage[1], batch, k_special,
                                          alpha, level, flags, (void *)ctx->hstream)))
    return rc;
  return s.out2(h_out0, h_out1, 2, ob);
}
int nflhip_mulrelin_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1,
                        const void *h_key, size_t batch, size_t k_special, size_t alpha, int flags) {
  int rc = mulrelin_check(ctx, h_out0, h_out1, h_a0, h_a1, h_b0, h_b1, h_key, batch, k_special, alpha, flags);
  if (rc || batch == 0) return rc;
  return mulrelin_host(ctx, h_out0, h_out1, h_a0, h_a1, h_b0, h_b1, h_key, batch, k_special, alpha, ctx->shape.nm - k_special, flags);
}
int nflhip_mulrelin_level_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1,
                              const void *h_key, size_t batch, size_t k_special, size_t alpha, size_t level, int flags) {
  int rc = level_check(ctx, k_special, level, "mulrelin");
  if (!rc) rc = mulrelin_check(ctx, h_out0, h_out1, h_a0, h_a1, h_b0, h_b1, h_key, batch, k_special, alpha, flags, level);
  if (rc || batch == 0) return rc;
  return mulrelin_host(ctx, h_out0, h_out1, h_a0, h_a1, h_b0, h_b1, h_key, batch, k_special, alpha, level, flags);
}

// sums of ciphertext products: a0, a1 dense [groups][terms] polynomials of `rows` rows, b0, b1 alike or [terms] with b_shared (both
// NULL: the squares).  The inputs share one slot (a0, a1, then b0, b1), the outputs another, as the tensor product above.
namespace {
struct TensorDotHost {
  size_t abytes, bbytes, nin;
  nflhip_dot_operand op[4];
};
}  // namespace
static int tensor_dot_host_sizes(nflhip_ctx *ctx, const char *what, const void *h_b0, size_t groups, size_t terms, int b_shared, size_t pbytes,
                                 TensorDotHost *h) {
  size_t polys, total;  // (the pointers are checked: the device entry's checks ran on these blocks)
  if (__builtin_mul_overflow(groups, terms, &polys) || __builtin_mul_overflow(polys, pbytes, &h->abytes) || __builtin_mul_overflow(h->abytes, (size_t)4, &total))
    return fail(ctx, NFLHIP_ERR_INVALID, std::string(what) + ": an operand's size overflows");
  h->bbytes = !h_b0 ? 0 : b_shared ? terms * pbytes : h->abytes;
  h->nin = h_b0 ? 4 : 2;
  return NFLHIP_OK;
}
// stage the inputs into slot 0 and describe them as the device entries take them
static int tensor_dot_host_stage(nflhip_ctx *ctx, Staged &s, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1, size_t terms,
                                 int b_shared, TensorDotHost *h) {
  int rc = s.in(0, nullptr, 2 * h->abytes + 2 * h->bbytes);
  if (rc) return rc;
  char *i = (char *)ctx->stage[0];
  const void *const hin[4] = {h_a0, h_a1, h_b0, h_b1};
  const size_t len[4] = {h->abytes, h->abytes, h->bbytes, h->bbytes}, off[4] = {0, h->abytes, 2 * h->abytes, 2 * h->abytes + h->bbytes};
  for (size_t k = 0; k < h->nin; ++k) {
    if (ctx->stage_host[0]) std::memcpy(i + off[k], hin[k], len[k]);
    else HIPCHK(ctx, hipMemcpyAsync(i + off[k], hin[k], len[k], hipMemcpyHostToDevice, ctx->hstream));
    h->op[k] = {i + off[k], k >= 2 && b_shared ? (size_t)0 : terms, 1};
  }
  return NFLHIP_OK;
}
int nflhip_tensor_dot_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, void *h_out2, const void *h_a0, const void *h_a1, const void *h_b0,
                          const void *h_b1, size_t groups, size_t terms, int b_shared, size_t rows, int flags) {
  // the device entry's checks on the host blocks, which lie as dense operands do
  const nflhip_dot_operand ha0 = {h_a0, terms, 1}, ha1 = {h_a1, terms, 1}, hb0 = {h_b0, b_shared ? (size_t)0 : terms, 1}, hb1 = {h_b1, b_shared ? (size_t)0 : terms, 1};
  int rc = tensor_dot_check(ctx, h_out0, h_out1, h_out2, &ha0, &ha1, h_b0 ? &hb0 : nullptr, h_b1 ? &hb1 : nullptr, groups, terms, rows, flags);
  if (rc || groups == 0) return rc;
  const size_t pbytes = rows * ctx->shape.n * ctx->word;
  TensorDotHost h;
  if ((rc = tensor_dot_host_sizes(ctx, "tensor_dot", h_b0, groups, terms, b_shared, pbytes, &h)) || (rc = set_device(ctx))) return rc;
  const size_t ob = groups * pbytes;
  Staged s(ctx);
  if ((rc = tensor_dot_host_stage(ctx, s, h_a0, h_a1, h_b0, h_b1, terms, b_shared, &h)) || (rc = s.in(2, nullptr, 3 * ob))) return rc;
  char *o = (char *)ctx->stage[2];
  if ((rc = nflhip_tensor_dot_ntt_dev(ctx, o, o + ob, o + 2 * ob, &h.op[0], &h.op[1], h_b0 ? &h.op[2] : nullptr, h_b0 ? &h.op[3] : nullptr, groups, terms, rows,
                                      flags, (void *)ctx->hstream)))
    return rc;
  void *const hout[3] = {h_out0, h_out1, h_out2};
  return s.outs(hout, 3, 2, ob);
}
// the multiplication over them: staged as mulrelin_host, the operands as above
int nflhip_mulrelin_dot_ntt(nflhip_ctx *ctx, void *h_out0, void *h_out1, const void *h_a0, const void *h_a1, const void *h_b0, const void *h_b1,
                            const void *h_key, size_t groups, size_t terms, int b_shared, size_t k_special, size_t alpha, size_t level, int flags) {
  int rc = level_check(ctx, k_special, level, "mulrelin_dot");
  if (rc) return rc;
  const size_t nm = ctx->shape.nm, row = ctx->shape.n * ctx->word, pbytes = level * row;
  TensorDotHost h;
  // the device entry's checks on the host blocks, which lie as dense operands do
  const nflhip_dot_operand ha0 = {h_a0, terms, 1}, ha1 = {h_a1, terms, 1}, hb0 = {h_b0, b_shared ? (size_t)0 : terms, 1}, hb1 = {h_b1, b_shared ? (size_t)0 : terms, 1};
  if ((rc = mulrelin_dot_check(ctx, h_out0, h_out1, &ha0, &ha1, h_b0 ? &hb0 : nullptr, h_b1 ? &hb1 : nullptr, h_key, groups, terms, k_special, alpha, level, flags)) ||
      groups == 0)
    return rc;
  if ((rc = tensor_dot_host_sizes(ctx, "mulrelin_dot", h_b0, groups, terms, b_shared, pbytes, &h))) return rc;
  const size_t ib = groups * pbytes, ob = (flags & NFLHIP_MULRELIN_RESCALE) ? ib - groups * row : ib;
  if ((rc = set_device(ctx))) return rc;
  const size_t kb = 2 * keyswitch_level_digits(ctx, k_special, alpha, level) * nm * row;
  Staged s(ctx);
  if ((rc = tensor_dot_host_stage(ctx, s, h_a0, h_a1, h_b0, h_b1, terms, b_shared, &h)) || (rc = s.in(1, h_key, kb)) || (rc = s.in(2, nullptr, 2 * ob))) return rc;
  char *o = (char *)ctx->stage[2];
  if ((rc = nflhip_mulrelin_dot_ntt_dev(ctx, o, o + ob, &h.op[0], &h.op[1], h_b0 ? &h.op[2] : nullptr, h_b0 ? &h.op[3] : nullptr, ctx->stage[1], groups, terms,
                                        k_special, alpha, level, flags, (void *)ctx->hstream)))
    return rc;
  return s.out2(h_out0, h_out1, 2, ob);
}

// sums of products across polynomials: the operands are `terms` times the size of the result, so the call is staged whole
int nflhip_dot(nflhip_ctx *ctx, void *h_out, const void *h_a, const void *h_b, size_t groups, size_t terms, int b_shared) {
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (ctx->cyclic) return fail(ctx, NFLHIP_ERR_INVALID, "dot: not on a cyclic row context");
  if (terms == 0 || terms > 0xffffffffu) return fail(ctx, NFLHIP_ERR_INVALID, "dot: the number of terms is out of range");
  if (groups == 0) return NFLHIP_OK;
  if (!h_out || !h_a || !h_b) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  size_t polys, abytes;
  if (__builtin_mul_overflow(groups, terms, &polys) || __builtin_mul_overflow(polys, poly_bytes(ctx, 1), &abytes))
    return fail(ctx, NFLHIP_ERR_INVALID, "dot: an operand's size overflows");
  const size_t obytes = poly_bytes(ctx, groups), bbytes = b_shared ? poly_bytes(ctx, terms) : abytes;
  if (ranges_overlap(h_out, obytes, h_a, abytes) || ranges_overlap(h_out, obytes, h_b, bbytes))
    return fail(ctx, NFLHIP_ERR_INVALID, "dot: the output overlaps an operand");
  int rc = set_device(ctx);
  if (rc) return rc;
  const HostIn ins[] = {{0, h_a, abytes}, {1, h_b, bbytes}};
  return staged_call(ctx, groups, false, ins, 2, {2, h_out, obytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    const nflhip_dot_operand a = {d[0], terms, 1}, b = {d[1], b_shared ? 0 : terms, 1};
    return nflhip_dot_dev(ctx, o, &a, &b, nullptr, cnt, terms, 0, st);
  });
}

// gadget decomposition: the result is `terms` times the input (or a compact fraction of that), so the call is staged whole
int nflhip_decompose(nflhip_ctx *ctx, void *h_out, int out_format, const void *h_in, size_t batch, int w, int flags) {
  if (out_format < 0) return fail(ctx, NFLHIP_ERR_INVALID, "decompose: unknown output format");
  size_t obytes = 0;
  int rc = decompose_check(ctx, h_out, out_format, h_in, batch, w, flags, &obytes);
  if (rc || batch == 0) return rc;
  if ((rc = set_device(ctx))) return rc;
  const HostIn ins[] = {{0, h_in, poly_bytes(ctx, batch)}};
  return staged_call(ctx, batch, false, ins, 1, {1, h_out, obytes}, [&](const void *const *d, void *o, size_t cnt, void *st) {
    return nflhip_decompose_dev(ctx, o, out_format, d[0], cnt, w, flags, st);
  });
}

int nflhip_ntt_row(nflhip_ctx *ctx, void *h_rows, size_t cm, int mode, size_t rows) {
  CHECK_CTX(ctx);
  if (rows == 0) return NFLHIP_OK;
  if (!h_rows) return fail(ctx, NFLHIP_ERR_INVALID, "NULL data pointer");
  const size_t bytes = rows * ctx->shape.n * ctx->word;
  const HostIn ins[] = {{0, h_rows, bytes}};
  return staged_call(ctx, rows, false, ins, 1, {0, h_rows, bytes}, [&](const void *const *, void *o, size_t cnt, void *st) {
    return nflhip_ntt_row_dev(ctx, o, cm, mode, cnt, st);
  });
}

int nflhip_pointwise(nflhip_ctx *ctx, int op, void *o, const void *a, const void *b, const void *bp, size_t batch) {
  CHECK_CTX(ctx);
  if (op < 0 || op > 4) return fail(ctx, NFLHIP_ERR_INVALID, "unknown element-wise op");
  if (batch == 0) return NFLHIP_OK;
  if (!o || !a || (op != NFLHIP_OP_COMPUTE_SHOUP && !b) || (op == NFLHIP_OP_MUL_SHOUP && !bp))
    return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t bytes = poly_bytes(ctx, batch);
  const HostIn ins[] = {{0, a, bytes}, {1, op != NFLHIP_OP_COMPUTE_SHOUP ? b : nullptr, bytes}, {2, op == NFLHIP_OP_MUL_SHOUP ? bp : nullptr, bytes}};
  return staged_call(ctx, batch, true, ins, 3, {0, o, bytes}, [&](const void *const *d, void *out, size_t cnt, void *st) {
    return nflhip_pointwise_dev(ctx, op, out, d[0], d[1], d[2], cnt, st);
  });
}

int nflhip_eval(nflhip_ctx *ctx, void *h_out, const void *const *h_operands, size_t noperands, const unsigned char *program,
                size_t proglen, size_t batch) {
  CHECK_CTX(ctx);
  if (!program || !h_operands) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (noperands == 0 || noperands > 4 || proglen == 0 || proglen > NFLHIP_EXPR_MAX_LEN)
    return fail(ctx, NFLHIP_ERR_UNSUPPORTED, "host-pointer eval takes at most 4 distinct operands");
  if (batch == 0) return NFLHIP_OK;
  if (!h_out) return fail(ctx, NFLHIP_ERR_INVALID, "NULL output");
  const size_t bytes = poly_bytes(ctx, batch);
  HostIn ins[4];
  for (size_t i = 0; i < noperands; ++i) {
    if (!h_operands[i]) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
    ins[i] = {(int)i, h_operands[i], bytes};
  }
  // four operands (c = c + shoup(a * b, b'): the reference's FMA with a precomputed companion) fill the four staging buffers: the result
  // is written over the first one -- the evaluation is element-wise, `out` may alias an input.  (The pipeline's slots hold three
  // inputs and the result.)
  return staged_call(ctx, batch, noperands <= 3, ins, (int)noperands, {noperands == 4 ? 0 : 3, h_out, bytes},
                     [&](const void *const *d, void *out, size_t cnt, void *st) {
                       return nflhip_eval_dev(ctx, out, d, noperands, program, proglen, cnt, st);
                     });
}

int nflhip_polymul(nflhip_ctx *ctx, void *c, const void *a, const void *b, size_t batch) {
  CHECK_CTX(ctx);
  if (batch == 0) return NFLHIP_OK;
  if (!c || !a || !b) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t bytes = poly_bytes(ctx, batch);
  const HostIn ins[] = {{0, a, bytes}, {1, b, bytes}};
  return staged_call(ctx, batch, true, ins, 2, {0, c, bytes}, [&](const void *const *d, void *out, size_t cnt, void *st) {
    return nflhip_polymul_dev(ctx, out, d[0], d[1], cnt, st);
  });
}

static int any_cmp_host(nflhip_ctx *ctx, const void *a, const void *b, size_t batch, int want_eq, int *result) {
  CHECK_CTX(ctx);
  if (!result) return fail(ctx, NFLHIP_ERR_INVALID, "NULL result");
  if (batch == 0) { *result = 0; return NFLHIP_OK; }
  if (!a || !b) return fail(ctx, NFLHIP_ERR_INVALID, "NULL operand");
  const size_t bytes = poly_bytes(ctx, batch);
  const HostIn ins[] = {{0, a, bytes}, {1, b, bytes}};
  return staged_call(ctx, batch, false, ins, 2, {-1, nullptr, 0}, [&](const void *const *d, void *, size_t cnt, void *st) {
    return (want_eq ? nflhip_any_eq_dev : nflhip_any_neq_dev)(ctx, d[0], d[1], cnt, result, st);
  });
}
int nflhip_any_eq(nflhip_ctx *ctx, const void *a, const void *b, size_t batch, int *result) {
  return any_cmp_host(ctx, a, b, batch, 1, result);
}
int nflhip_any_neq(nflhip_ctx *ctx, const void *a, const void *b, size_t batch, int *result) {
  return any_cmp_host(ctx, a, b, batch, 0, result);
}

int nflhip_check_range(const nflhip_ctx *ctx, const void *h_data, size_t batch, int *bad) {
  // host words against the host copy of the moduli: an assertion about the CALLER's data, nothing is computed
  if (!ctx) return fail(nullptr, NFLHIP_ERR_INVALID, "ctx is NULL");
  if (!bad || (batch && !h_data)) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  const size_t n = ctx->shape.n, nm = ctx->shape.nm;
  int hit = 0;
  for (size_t r = 0; r < batch * nm && !hit; ++r) {
    const uint64_t p = ctx->h_P[r % nm];
    if (ctx->word == 8) { const uint64_t *w = (const uint64_t *)h_data + r * n; for (size_t i = 0; i < n; ++i) hit |= w[i] >= p; }
    else if (ctx->word == 4) { const uint32_t *w = (const uint32_t *)h_data + r * n; for (size_t i = 0; i < n; ++i) hit |= w[i] >= p; }
    else { const uint16_t *w = (const uint16_t *)h_data + r * n; for (size_t i = 0; i < n; ++i) hit |= w[i] >= p; }
  }
  *bad = hit ? 1 : 0;
  return NFLHIP_OK;
}

int nflhip_crt_lift(nflhip_ctx *ctx, uint64_t *limbs, const void *d, size_t batch) {
  CHECK_CTX(ctx);
  if (batch == 0) return NFLHIP_OK;
  if (!limbs || !d) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  const size_t lbytes = batch * ctx->shape.n * ctx->shape.crt_L * sizeof(uint64_t);
  const HostIn ins[] = {{0, d, poly_bytes(ctx, batch)}};
  return staged_call(ctx, batch, false, ins, 1, {1, limbs, lbytes}, [&](const void *const *s, void *o, size_t cnt, void *st) {
    return nflhip_crt_lift_dev(ctx, (uint64_t *)o, s[0], cnt, st);
  });
}
int nflhip_crt_project(nflhip_ctx *ctx, void *d, const uint64_t *limbs, size_t L_in, size_t batch) {
  CHECK_CTX(ctx);
  if (batch == 0) return NFLHIP_OK;
  if (!limbs || !d) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  if (L_in == 0) return fail(ctx, NFLHIP_ERR_INVALID, "L_in must be positive");
  const HostIn ins[] = {{1, limbs, batch * ctx->shape.n * L_in * sizeof(uint64_t)}};
  return staged_call(ctx, batch, false, ins, 1, {0, d, poly_bytes(ctx, batch)}, [&](const void *const *s, void *o, size_t cnt, void *st) {
    return nflhip_crt_project_dev(ctx, o, (const uint64_t *)s[0], L_in, cnt, st);
  });
}

int nflhip_sample(nflhip_ctx *ctx, void *d, size_t batch, int dist, uint64_t p0, uint64_t p1, const unsigned char *key,
                  uint64_t stream_id) {
  CHECK_CTX(ctx);
  if (batch == 0) return NFLHIP_OK;
  if (!d) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  return staged_call(ctx, batch, false, nullptr, 0, {0, d, poly_bytes(ctx, batch)}, [&](const void *const *, void *o, size_t cnt, void *st) {
    return nflhip_sample_dev(ctx, o, 0, cnt, dist, p0, p1, key, stream_id, st);
  });
}

int nflhip_sample_gauss(nflhip_ctx *ctx, void *d, size_t batch, const nflhip_gauss *g, uint64_t amplifier,
                        const unsigned char *key, uint64_t stream_id) {
  CHECK_CTX(ctx);
  if (batch == 0) return NFLHIP_OK;
  if (!d) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  return staged_call(ctx, batch, false, nullptr, 0, {0, d, poly_bytes(ctx, batch)}, [&](const void *const *, void *o, size_t cnt, void *st) {
    return nflhip_sample_gauss_dev(ctx, o, 0, cnt, g, amplifier, key, stream_id, st);
  });
}

int nflhip_gauss_noise(nflhip_ctx *ctx, int64_t *h_out, size_t count, const nflhip_gauss *g, const unsigned char *key,
                       uint64_t stream_id) {
  CHECK_CTX(ctx);
  if (count == 0) return NFLHIP_OK;
  if (!h_out) return fail(ctx, NFLHIP_ERR_INVALID, "NULL argument");
  return staged_call(ctx, count, false, nullptr, 0, {0, h_out, count * sizeof(int64_t)}, [&](const void *const *, void *o, size_t cnt, void *st) {
    return nflhip_gauss_noise_dev(ctx, (int64_t *)o, 0, cnt, g, key, stream_id, st);
  });
}

}  // extern "C"
