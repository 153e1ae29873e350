// nfl_hip/queue.hpp -- part of the drop-in header; include <nfl_hip/nfl.hpp> (or the reference's names under include/nfl*).
// the deferred queue: recording, the hand-over of a run to the queue's own thread, the life cycle of a run, and the C-ABI calls
// that the planned runs (queue_plan.hpp) become.
#ifndef NFL_HIP_QUEUE_HPP
#define NFL_HIP_QUEUE_HPP
#ifndef NFL_HIP_NFL_HPP
#error "include <nfl_hip/nfl.hpp>: the parts depend on each other in its order"
#endif
namespace nfl {
template <class T, size_t Degree, size_t NbModuli> class poly;
template <class T, size_t Degree, size_t NbModuli> class poly_p;
namespace detail {
inline std::atomic<bool> &deferred_flag();
}
inline void set_deferred(bool on) { detail::deferred_flag().store(on); }
namespace tests {
template <class P> class poly_tests_proxy;  // (poly.hpp:69-76) defined by the caller's test code, befriended below
}

namespace detail {
#ifdef NFL_HIP_REFERENCE_WORDS
static constexpr int dist_flags = NFLHIP_DIST_REFERENCE_WORDS;
#else
static constexpr int dist_flags = 0;
#endif

// ---------------------------------------------------------------- deferred execution of per-polynomial operations
// One polynomial is 4 workgroups of work: a kernel launched for it runs for ~15 us on an otherwise empty GPU, and code
// written against the reference issues exactly such operations in loops (tests/nfllib_demo_main_op.cpp:26-58: three
// Gaussian polynomials, three transforms and two fused multiply-adds per encryption, one polynomial at a time).  So
// operations on resident handles are not launched when they are called: they are appended to a per-ring queue, and
// when a value is needed on the host (or the queue is long) the queue runs as a few BATCHED launches:
//   * operations are levelled by their data dependencies (read-after-write, write-after-read, write-after-write on
//     the shared payloads), so everything inside a level is independent;
//   * inside a level, operations with the same signature (same expression program, same distribution and parameters,
//     same transform) form a group; operands that are the same polynomial throughout (a key) split groups;
//   * results that have no buffer yet get CONSECUTIVE buffers (context::acquire_many), so a loop's temporaries form
//     dense arrays; a group is cut into runs whose operands advance by constant strides and every run is ONE launch of
//     the batch entry points (nflhip_eval_strided_dev, nflhip_sample[_gauss]_seq_dev, nflhip_ntt_fwd/inv_dev).
// Results are bit-identical to immediate execution (the random constructors keep the stream id they took when they
// were called).  nfl::set_deferred(false) (or -DNFL_HIP_EAGER) launches every operation at once instead.
inline std::atomic<bool> &deferred_flag() {
#ifdef NFL_HIP_EAGER
  static std::atomic<bool> f(false);
#else
  static std::atomic<bool> f(true);
#endif
  return f;
}

// ---- the hand-over of a queue run to the queue's own thread and back.  ONE run is in flight at most; the protocol does not
// depend on the ring type: lazy<P> gives it the function that executes its run in flight.
class handover {
  alignas(64) std::atomic<int> st;   // 0: no run in flight; 1: the run is with the queue's thread; 2: it is done with it (retire() is due)
  std::atomic<bool> w_sleeping, u_sleeping, quit;
  alignas(64) std::mutex wm;
  std::condition_variable wcv, ucv;
  // (read by the recording thread at a hand-over only: behind the mutex, away from the line of `st` that the queue's thread polls)
  std::thread *th;             // the queue's thread, created by the first hand-over (leaked in a forked child, which has no such thread)
  long th_pid;
  bool th_failed;
  std::function<void()> run;   // executes the run in flight

  static void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
  }
  // until `st` is `want` (or, for the queue's thread, `quit`): spin, then sleep on `cv` with `sleeping` raised for the other side
  void await(int want, bool or_quit, std::atomic<bool> &sleeping, std::condition_variable &cv) {
    unsigned spins = 0;
    while (st.load(std::memory_order_acquire) != want && !(or_quit && quit.load(std::memory_order_relaxed))) {
      if (++spins < 20000) {   // (a loop hands over the next run within a fraction of a millisecond: worth a short spin)
        cpu_relax();
        continue;
      }
      std::unique_lock<std::mutex> lk(wm);
      sleeping.store(true, std::memory_order_seq_cst);
      cv.wait(lk, [&] { return st.load(std::memory_order_seq_cst) == want || (or_quit && quit.load()); });
      sleeping.store(false, std::memory_order_seq_cst);
    }
  }
  void worker() {
#if defined(__linux__) && defined(__GLIBC__)
    pthread_setname_np(pthread_self(), "nflhip-queue");
#endif
    for (;;) {
      await(1, true, w_sleeping, wcv);
      if (st.load(std::memory_order_acquire) != 1) return;   // quit
      run();
      st.store(2, std::memory_order_seq_cst);
      if (u_sleeping.load(std::memory_order_seq_cst)) {
        std::lock_guard<std::mutex> lk(wm);
        ucv.notify_all();
      }
    }
  }

 public:
  explicit handover(std::function<void()> f) : st(0), w_sleeping(false), u_sleeping(false), quit(false), th(nullptr), th_pid(0), th_failed(false), run(f) {}
  bool busy() const { return st.load(std::memory_order_relaxed) == 1; }
  // whether there is a thread to hand a run to (created here, the first time); under the queue's lock, like everything below
  bool have_thread() {
    if (th_failed) return false;
    if (th) return own_thread();   // (not in a forked child: the thread stayed with the parent; runs are executed by their callers there)
    try {
      th_pid = long(getpid());
      th = new std::thread([this] { worker(); });
    } catch (...) {
      th = nullptr;
      th_failed = true;
      return false;
    }
    return true;
  }
  bool own_thread() const { return th && th_pid == long(getpid()); }
  void post() {
    st.store(1, std::memory_order_seq_cst);
    if (w_sleeping.load(std::memory_order_seq_cst)) {
      std::lock_guard<std::mutex> lk(wm);
      wcv.notify_one();
    }
  }
  // waits for the run in flight, if any
  enum flight { none, done, orphaned };   // orphaned: this is a forked child, the run stayed with the parent's thread
  flight wait() {
    const int s = st.load(std::memory_order_acquire);
    if (s == 0) return none;
    if (s == 1 && th_pid != long(getpid())) return orphaned;
    await(2, false, u_sleeping, ucv);
    return done;
  }
  void retired() { st.store(0, std::memory_order_relaxed); }
  void stop() {   // (own_thread(), nothing in flight)
    {
      std::lock_guard<std::mutex> lk(wm);
      quit.store(true);
      wcv.notify_all();
    }
    th->join();
    delete th;
  }
};

template <class P> struct lazy : queue_kinds {
  typedef payload<P> pay_t;
  typedef typename pay_t::ctx_t ctx_t;
  typedef typename P::value_type T;
  typedef std::shared_ptr<pay_t> ptr_t;
  typedef plan<P> plan_t;
  typedef typename plan_t::op op;
  // ---- the recording side (under mu).  The three groups below sit on cache lines of their own: the queue's thread polls the
  // handshake's state and writes its statistics while the recording thread appends to q with every operation -- on one line that
  // costs the recorder a cross-core transfer per record (measured: the LWE loop recorded 2.5 times SLOWER with the groups interleaved).
  alignas(64) light_lock mu;
  std::vector<op> q;           // recorded operations
  std::vector<ptr_t> pins;     // the payloads they name, one reference each
  unsigned rec_run_;           // the recording run: bumped whenever the queue is handed to a queue run (payload::rec_run)
  std::atomic<unsigned> done_run_;  // the last recording run that has been retired (payload::queued)
  size_t next_run_;            // records at which the next run is handed to the queue's thread
  // ---- the handshake
  alignas(64) handover hand;
  // ---- the executing side
  // The queue run in flight: the records and pins of one recording run (their vectors swap with q / pins: no regrowth), from
  // take() to retire().  Between hand.post() and the moment the queue's thread is done with it, it belongs to that thread;
  // otherwise to whoever holds `mu`.
  struct alignas(64) run_t {
    std::vector<op> ops, work;
    bool remote;               // executed by the queue's thread
    std::vector<ptr_t> held;
    std::vector<unsigned char> launched;
    // per pin, filled by take() (recording thread; nothing is in flight then, so every payload's `dev` is final): the value's
    // buffer (nullptr: none yet -- the run assigns one to its results and retire() writes it back) and whether the run's pin is
    // the LAST reference (no handle left: what the transform fusion needs to know before it lets a temporary never exist)
    std::vector<void *> dev;
    std::vector<unsigned char> dead;
    std::vector<int> wlev, rlev, fw;   // the run's levelling scratch, per pin
    unsigned char key[32];     // the sampler key as it was when the run was taken: set_sampler_key runs the queues before it changes it
    unsigned id;               // its recording run (payload::qrun)
    bool complete;
    std::exception_ptr error;  // what stopped it (rethrown by retire())
    run_t() : remote(false), id(0), complete(false) {}
  } fly;
  std::atomic<size_t> launches, coalesced;  // statistics: launches issued / operations they carried
  std::atomic<size_t> fused_fwd, fused_inv;  // statistics: sequences rewritten so far
  // compact Gaussian polynomials of a fused run live in ONE grow-only device buffer (every consumer is on the queue's stream)
  void *small_;
  size_t small_cap_;
  alignas(64) char pad_[64];   // (the executing side ends on a line of its own: whatever follows this object is not ours to slow down)
  // records after which the queue runs by itself: long enough for wide launches, short enough that the device works on
  // one part of a loop while the host records the next (NFL_HIP_QUEUE_LIMIT overrides, for experiments).  Measured on the
  // LWE demo loop (profiles/r02_late_queue_limit.txt): 2 048 iterations 614 k / 738 k / 1.04 M / 861 k encryptions/s with
  // 2 048 / 4 096 / 8 192 / 16 384 records, 16 384 iterations 1.09 M / 1.21 M / 1.16 M / 1.16 M with 4 096 ... 32 768.
  static size_t max_queue() {
    static const size_t v = getenv("NFL_HIP_QUEUE_LIMIT") ? size_t(atol(getenv("NFL_HIP_QUEUE_LIMIT"))) : 8192;
    return v ? v : 1;
  }
  // ---- the queue's own thread (round 6).  Preparing a queue run -- fusing, levelling, grouping, finding the stride runs -- and
  // issuing its launches cost the recording thread as much as the recording itself (tools/hostprof: 0.2 us of 0.43 us per LWE
  // encryption).  A run that starts because the queue is long enough is therefore handed to a thread of the queue's own:
  // the recording thread swaps in the other pair of vectors and goes on recording while that thread works.  ONE run is in flight
  // at most; the recording thread retires it (drops the pins, rethrows what stopped it) when it hands over the next one or when
  // anything needs the queue empty.  A run that somebody WAITS for (flush(): a value is read on the host, synchronize()) is
  // executed by the waiting thread itself once the one in flight is retired: no hand-over latency on short programs.
  // With a thread to hand runs to, the queue does not wait for max_queue() records either: from min_run() records on it hands
  // over as soon as the thread is idle, so the device starts on a loop's first part while the host is still recording
  // (the 2 048-iteration LWE loop used to leave the device idle for four fifths of its recording).
  // NFL_HIP_QUEUE_THREAD=0 (or a machine with one hardware thread, or a thread that cannot be created): every run is executed by
  // the thread that starts it, as before.  Results are identical either way (tests/cpp: deferred == immediate under both).
  static bool threaded() {
    static const bool v = getenv("NFL_HIP_QUEUE_THREAD") ? atoi(getenv("NFL_HIP_QUEUE_THREAD")) != 0 : std::thread::hardware_concurrency() > 1;
    return v;
  }
  static size_t min_run() {
    static const size_t v = getenv("NFL_HIP_QUEUE_MIN") ? size_t(atol(getenv("NFL_HIP_QUEUE_MIN"))) : 1024;
    return v ? v : 1;
  }
  // (Round 5 measured two run-length policies for SHORT loops and dropped both -- LWE demo loop, encryptions/s against the fixed
  //  length: a loop's first two runs at HALF length: 2 048 iterations 1.68 -> 1.85 M, but 1 024: 1.60 -> 1.39 M, 4 096: 2.12 ->
  //  2.08 M, 16 384: 2.48 -> 2.43 M; its first run at THREE QUARTERS: 2 048: 1.67 -> 1.88 M, 4 096: 2.10 -> 2.16 M, but 1 536:
  //  1.67 -> 1.60 M, 3 072: 2.01 -> 1.86 M.  Any fixed threshold moves the sawtooth, it does not remove it: what a short loop
  //  pays beyond its recording is the device work that starts when the loop ends.  The host records an encryption in 0.36 us
  //  and a run costs it ~36 us, so 2.78 M/s is the ceiling of ANY policy at 2 048 iterations: profiles/r05_short_loops.txt.)

  // NFL_HIP_EARLY_RUN=1: from 1 024 records on, every 512 records the queue asks whether the stream is idle
  // (nflhip_stream_idle: one hipStreamQuery) and runs at once if it is.  Off by default: measured on the LWE demo's
  // 2 048-iteration loop it changes nothing (profiles/r02_late_early_run.txt); results are identical either way.
  static bool early_run() {
    static const bool v = getenv("NFL_HIP_EARLY_RUN") && atoi(getenv("NFL_HIP_EARLY_RUN")) != 0;
    return v;
  }
  lazy() : rec_run_(1), done_run_(0), next_run_(std::min(min_run(), max_queue())), hand([this] { execute(fly); }),
           launches(0), coalesced(0), fused_fwd(0), fused_inv(0), small_(nullptr), small_cap_(0) {
    ctx_t::inst();  // (the context is constructed first, so it is destroyed last)
    alive() = true;
    queue_registry::get().add(&lazy::run_if_alive);
  }
  ~lazy() {
    alive() = false;
    if (hand.own_thread()) {
      try {   // the run in flight holds raw pointers into this object: see it out (what it reports has nobody to go to)
        std::lock_guard<light_lock> lk(mu);
        collect();
      } catch (...) {
      }
      hand.stop();
    }
    if (small_ && ctx_t::alive()) nflhip_free(ctx_t::get(), small_);
  }
  static bool &alive() {
    static bool a = false;
    return a;
  }
  static void run_if_alive() {  // what queue_registry calls (possibly while the program's statics are being destroyed)
    if (alive() && ctx_t::alive()) inst().flush();
  }
  static lazy &inst() {
    static lazy l;
    return l;
  }
  // whether a run rewrites transform sequences (plan<P>::fuse): the context has the fused kernels, and NFL_HIP_NO_FUSION is not set
  static bool fusion_on() {
    static const bool v = !getenv("NFL_HIP_NO_FUSION") && nflhip_has_fused_kernels(ctx_t::get()) != 0;
    return v;
  }
  void *small_buffer(size_t bytes) {
    if (bytes > small_cap_) {
      nflhip_ctx *c = ctx_t::get();
      if (small_) {
        check(c, nflhip_stream_sync(c, ctx_t::queue()), "compact sampler buffer");   // (its last readers)
        nflhip_free(c, small_);
        small_ = nullptr;
        small_cap_ = 0;
      }
      size_t cap = size_t(1) << 20;
      while (cap < bytes) cap *= 2;
      check(c, nflhip_malloc(c, &small_, cap), "compact sampler buffer");
      small_cap_ = cap;
    }
    return small_;
  }
  // the narrowest compact format that holds every sample of `tab` times `amp` (NFLHIP_FMT_I8 / I16 / I32; 99 = none)
  static int small_format(const nflhip_gauss *tab, uint32_t amp) {
    struct last_t { const nflhip_gauss *tab; uint64_t mag; };
    static thread_local last_t last = {nullptr, 0};
    if (last.tab != tab) {
      long long x_min = 0;
      size_t entries = 0;
      check(ctx_t::get(), nflhip_gauss_info(tab, &x_min, &entries, nullptr, nullptr, nullptr, nullptr), "gaussian table");
      const long long hi = x_min + (long long)entries - 1;
      last.tab = tab;
      last.mag = uint64_t(std::max(x_min < 0 ? -x_min : x_min, hi < 0 ? -hi : hi));
    }
    const uint64_t v = last.mag * uint64_t(amp);
    return v <= 127 ? NFLHIP_FMT_I8 : v <= 32767 ? NFLHIP_FMT_I16 : v <= 2147483647ull ? NFLHIP_FMT_I32 : 99;
  }
  // whether this ring's operations can be deferred at all: dense chunks, vectors of 16 bytes, sequence samplers
  static bool usable() {
    return deferred_flag().load(std::memory_order_relaxed) && ctx_t::chunk_bytes == ctx_t::poly_bytes && P::degree >= 8 &&
           P::degree * sizeof(T) >= 16;
  }
  // the recording run's reference to a payload, taken the first time one of its operations mentions it (the recording scratch
  // is tagged with the run at the same moment: "mentioned in this run" and "pinned by this run" are one fact)
  pay_t *pin(pay_t *p) {
    if (p->rec_run != rec_run_) {
      p->rec_run = rec_run_;
      p->rec_w = p->rec_r = -1;
      p->pin_at = unsigned(pins.size());
      pins.push_back(p->shared_from_this());
      ++p->qrefs;
    }
    return p;
  }
  // A transform recorded on a value that a Gaussian constructor or an expression of THIS recording run produced and that
  // nothing has read since does not become a record of its own: the producing operation notes "then transform in place"
  // (op::post).  The reference's loops are written that way -- poly_p u{gaussian}; u.ntt_pow_phi();  out = rb - ra * s;
  // out.invntt_pow_invphi(); -- and every record costs the host the same whatever it stands for.  Results are those of the
  // separate records; NFL_HIP_NO_FUSION=1 switches this off together with the transform fusion.
  static bool joining_on() {
    static const bool v = !getenv("NFL_HIP_NO_FUSION");
    return v;
  }
  bool join_transform(pay_t *p, int kind) {
    if (!joining_on()) return false;
    std::lock_guard<light_lock> lk(mu);
    if (p->rec_run != rec_run_ || p->rec_w < 0 || p->rec_r > p->rec_w || p->poisoned) return false;
    op &t = q[size_t(p->rec_w)];
    if (t.post || t.out != p || !((t.kind == K_GAUSS && kind == K_NTT_FWD) || t.kind == K_EVAL)) return false;
    t.post = static_cast<unsigned char>(kind);
    return true;
  }
  // a record enters the recording run at index `at`: the payloads it names are pinned, and remember it as their last reader / writer
  void enlist(op &o, int at) {
    plan_t::for_each_pin(o, [&](pay_t *p, unsigned &k) { pin(p)->rec_r = at; k = p->pin_at; },
                         [&](pay_t *p, unsigned &k) { pin(p)->rec_w = at; k = p->pin_at; p->qrun = rec_run_; });
  }
  // `fill(op &)` writes the record in place, in the queue; the payloads it names are pinned here
  template <class F> void record(F fill) {
    std::lock_guard<light_lock> lk(mu);
    q.emplace_back();
    op &o = q.back();
#if defined(__x86_64__)
    // the vector's storage was last read by the queue's thread (another core, often another L3): ask for the lines this loop will
    // write a dozen records from now in exclusive state NOW, so that the stores do not each wait for the invalidation
    if (q.size() + 16 <= q.capacity()) {
      const char *ahead = reinterpret_cast<const char *>(&o + 16);
      __asm__ volatile("prefetchw %0\n\tprefetchw %1" : : "m"(*ahead), "m"(*(ahead + 64)));
    }
#endif
    o.nin = 0;
    o.len = 0;
    o.post = 0;
    try {  // what it reads must hold a device value (or be produced by the queue) before the operation counts as recorded
      fill(o);
      plan_t::for_each_pin(o, [](pay_t *p, unsigned &) { p->dev_ro_nf(); }, [](pay_t *, unsigned &) {});
    } catch (...) {
      q.pop_back();
      throw;
    }
    enlist(o, int(q.size()) - 1);
    o.out->dev_valid = true;
    o.out->host_valid = false;
    if (o.kind != K_NTT_FWD && o.kind != K_NTT_INV) o.out->poisoned = false;  // overwritten entirely
    const size_t n = q.size();
    if (!threaded()) {
      if (n >= max_queue()) hand_over();
    } else if (n >= next_run_ && (n >= 2 * max_queue() || (n % 64 == 0 && !hand.busy())) && have_thread()) {
      // Run lengths of a loop grow geometrically (min_run(), twice that, ... up to max_queue()): the device starts on the loop's
      // first few hundred iterations while the host is still recording, and the later runs are long enough for the device's
      // best rate (per run it pays three sampler launches and the drain of the fused kernel, whatever the length).  A run waits
      // for the queue's thread only at twice the full length; flush() -- somebody waited: the loop is over -- starts anew.
      hand_over();
      next_run_ = std::min(next_run_ * 2, max_queue());
    } else if (n >= 2 * max_queue()) {
      hand_over();   // (no thread after all)
    } else if (early_run() && n >= 1024 && n % 512 == 0) {
      // a loop shorter than the queue: do not let the device sit idle until the loop's end
      int idle = 0;
      if (nflhip_stream_idle(ctx_t::get(), ctx_t::queue(), &idle) == NFLHIP_OK && idle) hand_over();
    }
  }
  // everything recorded so far has been launched (or has failed: rethrown here) when this returns
  void flush() {
    std::lock_guard<light_lock> lk(mu);
    next_run_ = std::min(min_run(), max_queue());
    collect();
    if (q.empty()) return;
    take();
    execute(fly);   // somebody waits for it: no hand-over
    retire();
  }
  // the records so far become the run in flight (the previous one is retired first): on the queue's thread if there is one
  void hand_over() {
    collect();
    if (q.empty()) return;
    take(clean_cut());
    if (have_thread()) {
      fly.remote = true;
      hand.post();
    } else {
      execute(fly);
      retire();
    }
  }
  bool have_thread() { return threaded() && hand.have_thread(); }   // (under mu)
  // Where to cut the queue when a run starts by itself in the middle of a loop.  The iteration that is being recorded right now has
  // sampled its temporaries but not consumed them yet (poly_p u{gaussian}; u.ntt_pow_phi(); ra = u * pka + e1; | rb = u * pkb + e2;):
  // a run that takes its first half cannot fuse it -- u has a handle and another reader to come -- and launches nine small
  // kernels for that one iteration instead (a fifth of the device's time per run, rocprofv3 timeline of the LWE loop).  So the
  // records from the first one that mentions a Gaussian temporary of the last few records whose HANDLE IS STILL ALIVE stay in
  // the queue for the next run.  -> number of records the run takes (all of them when there is no such temporary).
  size_t clean_cut() const {
    const size_t n = q.size(), window = 32;
    const size_t from = n > window ? n - window : 0;
    unsigned open_pin[8];
    int nopen = 0;
    for (size_t i = from; i < n && nopen < 8; ++i) {
      const op &o = q[i];
      if (o.kind == K_GAUSS && pins[o.out_pin].use_count() - o.out->qrefs >= 1) open_pin[nopen++] = o.out_pin;
    }
    if (!nopen) return n;
    for (size_t i = from; i < n; ++i)
      for (int k = 0; k < nopen; ++k)
        if (plan_t::mentions(q[i], open_pin[k])) return i ? i : n;   // (nothing in front of it: take everything)
    return n;
  }
  void take(size_t cut = size_t(-1)) {   // (under mu, nothing in flight); records from `cut` on stay in the queue
    op rest[32];
    size_t nrest = 0;
    if (cut < q.size()) {
      nrest = q.size() - cut;
      std::copy(q.begin() + ptrdiff_t(cut), q.end(), rest);
      q.resize(cut);
    }
    fly.ops.swap(q);
    fly.held.swap(pins);
    if (q.capacity() < fly.ops.capacity()) q.reserve(fly.ops.capacity());
    fly.id = rec_run_++;   // (what is recorded from now on cannot join operations of this run, and pins again)
    for (size_t i = 0; i < nrest; ++i) {   // the records that stay: recorded again, in the new recording run
      q.push_back(rest[i]);
      enlist(q.back(), int(q.size()) - 1);
    }
    fly.launched.assign(fly.ops.size(), 0);
    const size_t np = fly.held.size();
    fly.dev.resize(np);
    fly.dead.resize(np);
    for (size_t k = 0; k < np; ++k) {
      fly.dev[k] = fly.held[k]->dev;
      fly.dead[k] = fly.held[k].use_count() == 1;
    }
    fly.complete = false;
    fly.error = nullptr;
    fly.remote = false;
    detail::sampler::get().copy_key(fly.key);
  }
  // wait for the run in flight, if any, and retire it (under mu)
  void collect() {
    const handover::flight f = hand.wait();
    if (f == handover::none) return;
    if (f == handover::orphaned) {
      fly.complete = false;
      fly.error = std::make_exception_ptr(std::runtime_error("nfl(hip): the process forked while a queue run was in flight"));
    }
    retire();
  }
  // the run in flight is over (under mu; executed here, or by the queue's thread which has set st = 2): its values stop being
  // queued, its references go; if a launch failed, what was never launched holds no value -- later accesses throw
  // (payload::usable) -- and so does everything recorded since (it was recorded on top of values that do not exist): rethrown
  void retire() {
    hand.retired();
    done_run_.store(fly.id, std::memory_order_relaxed);
    const bool failed = !fly.complete;
    if (failed)
      for (size_t i = 0; i < fly.ops.size(); ++i)
        if (!fly.launched[i]) {
          fly.ops[i].out->dev_valid = false;
          fly.ops[i].out->poisoned = true;
        }
    fly.ops.clear();
    for (size_t k = 0; k < fly.held.size(); ++k) {
      pay_t *p = fly.held[k].get();
      p->dev = fly.dev[k];   // (results that had no buffer got theirs from the run)
      --p->qrefs;
    }
    if (failed && !q.empty()) {
      for (auto &o : q) {
        o.out->dev_valid = false;
        o.out->poisoned = true;
      }
      q.clear();
      for (auto &p : pins) --p->qrefs;
      fly.held.insert(fly.held.end(), pins.begin(), pins.end());
      pins.clear();
      done_run_.store(rec_run_++, std::memory_order_relaxed);
    }
    if (ctx_t::alive()) {   // the temporaries' buffers go back to the pool one by one: its lock is taken once for all of them
      std::lock_guard<light_lock> pool(ctx_t::inst().mu);
      fly.held.clear();
    } else {
      fly.held.clear();
    }
    if (failed) {
      std::exception_ptr e = fly.error;
      fly.error = nullptr;
      if (e) std::rethrow_exception(e);
      throw std::runtime_error("nfl(hip): a deferred operation failed");
    }
  }
  // One queue run: fuse, level, group, launch.  Runs on the queue's thread or on the thread that waits for it; touches nothing
  // of the recording state (see payload: `dev` of results without a buffer, and the levelling scratch).  Never throws: what
  // stops it is kept in r.error, r.launched says which operations were issued.
  void execute(run_t &r) {
    static const bool stats = getenv("NFL_HIP_TRACE_DEFERRED") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nops = r.ops.size();
    try {
      execute_body(r);
      r.complete = true;
    } catch (...) {
      r.error = std::current_exception();
    }
    if (stats) {
      const double us = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e6;
      std::fprintf(stderr, "nfl(hip) queue run: %zu records in %.1f us (%s)\n", nops, us, r.remote ? "the queue's thread" : "the calling thread");
    }
  }
  // One queue run, planned by queue_plan.hpp: fuse, level, group; then per group, level by level: buffers, launches.
  void execute_body(run_t &r) {
    // The queue's thread works on a COPY of the records: it rewrites them (fusion), and lines it has written would have to come
    // back from its cache, one by one, when the recording thread fills the same vector again two runs later.
    if (r.remote) r.work.assign(r.ops.begin(), r.ops.end());
    std::vector<op> &ops = r.remote ? r.work : r.ops;
    if (ops.size() >= 2 && fusion_on()) plan_t::fuse(ops, r.fw, r.dead, &lazy::small_format, fused_fwd, fused_inv);
    std::vector<int> lvl;
    plan_t::level(ops, r.wlev, r.rlev, r.held.size(), lvl);
    for (size_t i = 0; i < ops.size(); ++i)
      if (lvl[i] < 0) r.launched[i] = 1;   // (K_NOP)
    std::vector<typename plan_t::group> groups;
    std::vector<size_t> order;
    plan_t::group_by_signature(ops, lvl, groups, order);
    for (size_t gi : order) run_group(r, ops, groups[gi]);
  }
  void run_group(run_t &r, const std::vector<op> &ops, typename plan_t::group &g) {
    static const bool trace = getenv("NFL_HIP_TRACE_DEFERRED") != nullptr;
    std::vector<size_t> &idx = g.idx;
    const int kind = ops[idx[0]].kind, nin = ops[idx[0]].nin;
    struct tracer {
      bool on; int level, kind; size_t n; const std::atomic<size_t> &now; size_t before;
      ~tracer() { if (on) std::fprintf(stderr, "nfl(hip) deferred: level %d kind %d: %zu operations -> %zu launches\n", level, kind, n, now.load() - before); }
    } tr{trace, g.level, kind, idx.size(), launches, launches};
    if ((kind == K_SAMPLE || kind == K_GAUSS) && idx.size() >= 4) plan_t::regroup_periodic(ops, idx);
    assign_buffers(ops, idx, r.dev);
    if (kind == K_NTT_FWD || kind == K_NTT_INV) {
      launch_transforms(r, ops, idx, kind);
    } else if (kind == K_FILL) {
      for (size_t i : idx) {
        check(ctx_t::get(), nflhip_fill_uniform_dev(ctx_t::get(), r.dev[ops[i].out_pin], 0, 1, ops[i].s.sid, 0, ctx_t::queue()), "deferred set(uniform)");
        r.launched[i] = 1;
        ++launches;
        ++coalesced;
      }
    } else if (kind == K_SAMPLE || kind == K_GAUSS) {
      launch_samplers(r, ops, idx);
    } else {   // K_EVAL and the fused kinds, whose operands sit in the same slots: key operands split the group, then stride runs
      std::vector<typename plan_t::subgroup> sub;
      plan_t::split_by_keys(ops, idx, nin, sub);
      for (auto &sv : sub)
        if (kind == K_FWD_FMA) launch_fwd_fma(r, ops, sv.idx);
        else launch_eval(r, ops, sv.idx);
    }
    // (operations that carry a joined transform count as launched only once it has been issued)
    const int post = ops[idx[0]].post;
    if (!post) return;
    for (size_t i : idx) r.launched[i] = 0;
    launch_transforms(r, ops, idx, post);
  }
  // buffers for results that have none yet: consecutive, in program order; the second results of K_FWD_FMA: a dense array of their own
  static void assign_buffers(const std::vector<op> &ops, const std::vector<size_t> &idx, std::vector<void *> &D) {
    for (int j = 0; j < (ops[idx[0]].kind == K_FWD_FMA ? 2 : 1); ++j) {
      std::vector<unsigned> need;
      for (size_t i : idx)
        if ((j == 0 || ops[i].f.out2) && !D[plan_t::result_pin(ops[i], j)]) need.push_back(plan_t::result_pin(ops[i], j));
      if (need.empty()) continue;
      std::vector<void *> bufs(need.size());
      ctx_t::acquire_many(need.size(), bufs.data());
      for (size_t k = 0; k < need.size(); ++k) D[need[k]] = bufs[k];
    }
  }
  // in-place transforms of the results of `idx` (mutually independent), which count as launched after the last of them:
  // by address, so that neighbours become one dense batch
  void launch_transforms(run_t &r, const std::vector<op> &ops, const std::vector<size_t> &idx, int tkind) {
    nflhip_ctx *ctx = ctx_t::get();
    std::vector<char *> ptr;
    ptr.reserve(idx.size());
    for (size_t i : idx) ptr.push_back(static_cast<char *>(r.dev[ops[i].out_pin]));
    plan_t::sort_interleaved(ptr);
    for (size_t a = 0; a < ptr.size();) {
      size_t b = a + 1;
      while (b < ptr.size() && ptr[b] == ptr[b - 1] + ctx_t::chunk_bytes) ++b;
      check(ctx, tkind == K_NTT_FWD ? nflhip_ntt_fwd_dev(ctx, ptr[a], b - a, ctx_t::queue()) : nflhip_ntt_inv_dev(ctx, ptr[a], b - a, ctx_t::queue()),
            "deferred transform");
      ++launches;
      coalesced += b - a;
      a = b;
    }
    for (size_t i : idx) r.launched[i] = 1;   // (all of them issued)
  }
  // idx as stride runs (plan<P>::extend_run), each ONE call of launch(first member, members, strides)
  template <class F> void for_each_run(run_t &r, const std::vector<op> &ops, const std::vector<size_t> &idx, int nres, int nin, int nsid, bool dense, F launch) {
    typename plan_t::strides s;
    for (size_t a = 0, b; a < idx.size(); a = b) {
      b = plan_t::extend_run(ops, idx, a, r.dev, nres, nin, nsid, dense, s);
      launch(ops[idx[a]], b - a, s);
      for (size_t k = a; k < b; ++k) r.launched[idx[k]] = 1;
      ++launches;
    }
  }
  static nflhip_operand operand(const void *ptr, size_t stride, int format) {
    const nflhip_operand o = {ptr, stride, format};
    return o;
  }
  // program order; a run = consecutive buffers + stream ids in arithmetic progression.  (r.key: the sampler key as it was when the run was taken)
  void launch_samplers(run_t &r, const std::vector<op> &ops, const std::vector<size_t> &idx) {
    nflhip_ctx *ctx = ctx_t::get();
    void *st = ctx_t::queue();
    for_each_run(r, ops, idx, 1, 0, 1, true, [&](const op &o0, size_t cnt, const typename plan_t::strides &s) {
      void *out = r.dev[o0.out_pin];
      if (o0.kind == K_SAMPLE)
        check(ctx, cnt == 1 ? nflhip_sample_dev(ctx, out, 0, 1, o0.s.dist, o0.s.p0, o0.s.p1, r.key, o0.s.sid, st)
                            : nflhip_sample_seq_dev(ctx, out, cnt, o0.s.dist, o0.s.p0, o0.s.p1, r.key, o0.s.sid, s.sid[0], st),
              "deferred random constructor");
      else
        check(ctx, cnt == 1 ? nflhip_sample_gauss_dev(ctx, out, 0, 1, o0.s.tab, o0.s.p1, r.key, o0.s.sid, st)
                            : nflhip_sample_gauss_seq_dev(ctx, out, cnt, o0.s.tab, o0.s.p1, r.key, o0.s.sid, s.sid[0], st),
              "deferred set(gaussian)");
      coalesced += cnt;
    });
  }
  // program order; a run = consecutive result buffers (both results), keys at constant strides, stream ids of
  // every Gaussian operand in arithmetic progression: the samplers' compact outputs and ONE fused launch
  void launch_fwd_fma(run_t &r, const std::vector<op> &ops, const std::vector<size_t> &idx) {
    nflhip_ctx *ctx = ctx_t::get();
    void *st = ctx_t::queue();
    const std::vector<void *> &D = r.dev;
    const int nin = ops[idx[0]].nin, nx = nin + 1;   // one key per result; x and one e per result
    const bool two = nin == 2;
    for_each_run(r, ops, idx, nin, nin, nx, true, [&](const op &o0, size_t cnt, const typename plan_t::strides &s) {
      int fmt = NFLHIP_FMT_I8;
      for (int j = 0; j < nx; ++j) fmt = std::max(fmt, small_format(o0.f.tab, o0.f.amp[j]));
      const size_t es = fmt == NFLHIP_FMT_I8 ? 1 : fmt == NFLHIP_FMT_I16 ? 2 : 4, each = (cnt * P::degree * es + 255) / 256 * 256;
      char *buf = static_cast<char *>(small_buffer(each * size_t(nx)));
      nflhip_operand x[3], k[2];
      void *dst[3];
      uint64_t amp[3];
      for (int j = 0; j < nx; ++j) {
        dst[j] = buf + each * size_t(j);
        amp[j] = o0.f.amp[j];
        x[j] = operand(dst[j], 1, fmt);
      }
      // (x, e0, e1 of a fused record are draws of ONE table: one launch for the three)
      check(ctx, nflhip_sample_gauss_small_multi_dev(ctx, dst, size_t(nx), fmt, cnt, o0.f.tab, amp, r.key, o0.f.sid, s.sid, st),
            "deferred set(gaussian), compact");
      ++launches;
      for (int j = 0; j < nin; ++j) k[j] = operand(D[o0.in_pin[j]], cnt > 1 ? s.in[j] : 0, NFLHIP_FMT_WORDS);
      check(ctx, two ? nflhip_fwd_fma2_dev(ctx, D[o0.out_pin], D[o0.f.out2_pin], &x[0], &k[0], &x[1], &k[1], &x[2], cnt, st)
                     : nflhip_fwd_fma_dev(ctx, D[o0.out_pin], &x[0], &k[0], &x[1], cnt, st),
            "deferred transform + multiply-add");
      coalesced += cnt * (two ? 8 : 5);   // (the operations the run's members were recorded as)
    });
  }
  // K_EVAL / K_FMA_INV, by destination address; a run = results and operands at constant strides (the fused entry writes dense results)
  void launch_eval(run_t &r, const std::vector<op> &ops, std::vector<size_t> &idx) {
    nflhip_ctx *ctx = ctx_t::get();
    void *st = ctx_t::queue();
    const std::vector<void *> &D = r.dev;
    const int kind = ops[idx[0]].kind, nin = ops[idx[0]].nin;
    plan_t::sort_by_result(ops, idx, D);
    for_each_run(r, ops, idx, 1, nin, 0, kind == K_FMA_INV, [&](const op &o0, size_t cnt, const typename plan_t::strides &s) {
      const void *d[NFLHIP_EXPR_MAX_OPERANDS];
      for (int j = 0; j < nin; ++j) d[j] = D[o0.in_pin[j]];
      if (kind == K_FMA_INV) {   // in[0] +- in[1] * in[2], then the inverse transform: one launch
        nflhip_operand w[3];
        for (int j = 0; j < 3; ++j) w[j] = operand(d[j], cnt > 1 ? s.in[j] : 0, NFLHIP_FMT_WORDS);
        check(ctx, nflhip_fma_inv_dev(ctx, D[o0.out_pin], &w[1], &w[2], &w[0], o0.e.code[0], cnt, st), "deferred multiply-add + inverse transform");
        coalesced += cnt;   // (two recorded operations per member)
      } else if (cnt == 1) {
        check(ctx, nflhip_eval_dev(ctx, D[o0.out_pin], d, size_t(nin), o0.e.code, size_t(o0.len), 1, st), "deferred operator=(expr)");
      } else {
        check(ctx, nflhip_eval_strided_dev(ctx, D[o0.out_pin], s.out, d, s.in, size_t(nin), o0.e.code, size_t(o0.len), cnt, st),
              "deferred operator=(expr)");
      }
      coalesced += cnt;
    });
  }
};
}  // namespace detail
}  // namespace nfl
#endif  // NFL_HIP_QUEUE_HPP

