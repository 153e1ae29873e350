// nfl_hip/payload.hpp -- part of the drop-in header; include <nfl_hip/nfl.hpp> (or the reference's names under include/nfl*).
// the shared payload of a resident poly_p handle and the per-thread block pool its control blocks come from.
#ifndef NFL_HIP_PAYLOAD_HPP
#define NFL_HIP_PAYLOAD_HPP
#ifndef NFL_HIP_NFL_HPP
#error "include <nfl_hip/nfl.hpp>: the parts depend on each other in its order"
#endif
namespace nfl {
namespace detail {
template <class P> struct lazy;

// Handle payloads come and go at the rate of the caller's temporaries (three per encryption of the LWE demo loop), and a
// general-purpose malloc / free pair per payload was the largest single item of the per-polynomial host cost (tools/hostprof:
// ~115 ns of ~185 per temporary).  std::allocate_shared with this allocator takes the control block + payload from a
// per-thread free list of fixed-size blocks instead; blocks freed on another thread simply join that thread's list.
template <class U> struct block_pool_alloc {
  typedef U value_type;
  block_pool_alloc() noexcept {}
  template <class V> block_pool_alloc(const block_pool_alloc<V> &) noexcept {}
  template <class V> struct rebind { typedef block_pool_alloc<V> other; };
  struct node { node *next; };
  struct list_t {
    node *head;
    size_t count;
    list_t() : head(nullptr), count(0) {}
    ~list_t() {
      gone() = true;   // (payloads released later in this thread's teardown -- static destructors -- go straight back to the heap)
      while (head) {
        node *n = head;
        head = n->next;
        ::operator delete(static_cast<void *>(n));
      }
      count = 0;
    }
  };
  static bool &gone() {   // trivially destructible, so it outlives the list it guards
    static thread_local bool g = false;
    return g;
  }
  static list_t &list() {
    static thread_local list_t l;
    return l;
  }
  U *allocate(size_t n) {
    if (n == 1 && sizeof(U) >= sizeof(node) && !gone()) {
      list_t &l = list();
      if (l.head) {
        node *x = l.head;
        l.head = x->next;
        --l.count;
        return reinterpret_cast<U *>(x);
      }
    }
    return static_cast<U *>(::operator new(n * sizeof(U)));
  }
  void deallocate(U *p, size_t n) noexcept {
    if (n == 1 && sizeof(U) >= sizeof(node) && !gone()) {
      list_t &l = list();
      if (l.count < (size_t(1) << 16)) {   // (bounded: a burst of 65 536 dead temporaries is kept, the rest goes back)
        node *x = reinterpret_cast<node *>(p);
        x->next = l.head;
        l.head = x;
        ++l.count;
        return;
      }
    }
    ::operator delete(static_cast<void *>(p));
  }
  template <class V> bool operator==(const block_pool_alloc<V> &) const noexcept { return true; }
  template <class V> bool operator!=(const block_pool_alloc<V> &) const noexcept { return false; }
};

// The shared payload of a poly_p handle (poly_p.hpp:11-204 keeps a std::shared_ptr<poly>): one polynomial that lives
// in HBM (`dev`), on the host (`host`), or both.  host_valid / dev_valid say which image holds the current value;
// neither valid = the zero polynomial (what poly_p() is) with nothing allocated yet.  Every device-side operation is
// enqueued on the context's stream, so the only synchronisation points are the device-to-host copies below.
// queued(): the value is the result of operations that are still in the deferred queue (lazy<P>, queue.hpp: recorded, or handed to
// a queue run that has not been retired yet); every access other than enqueueing more work runs the queue first (pending()).
// A queue run (lazy<P>::execute, possibly on the queue's own thread) never touches a payload: take() copies what it needs into
// per-run arrays and retire() writes the buffers it assigned back.  Every field belongs to the recording threads (under the
// queue's lock), which in turn leave `dev` of a queued value alone until its run is retired.
template <class P> struct payload : std::enable_shared_from_this<payload<P>> {
  typedef typename P::value_type T;
  typedef context<T, P::degree, P::nmoduli> ctx_t;
  static constexpr size_t bytes = sizeof(T) * P::degree * P::nmoduli;
  P *host;
  void *dev;
  bool host_valid, dev_valid;
  unsigned qrun;  // the recording run of the last deferred operation that writes this value (0: none); see queued()
  bool poisoned;  // the deferred operation that was to produce this value never ran (an earlier launch of its queue run failed)
  long qrefs;  // references the deferred queue holds to this value (one per queue run that mentions it: the one being recorded, the
              // one in flight): copy-on-write decisions look past them
  unsigned pin_at;  // where the recording run's reference to this payload sits in its pin list (valid while rec_run is the current one)
  // recording scratch of lazy<P>::record (valid when `rec_run` is the queue's current recording run): index of the last
  // recorded operation that writes / reads this value -- what lets a transform join the operation that produced its operand
  unsigned rec_run;
  int rec_w, rec_r;

  payload() : host(nullptr), dev(nullptr), host_valid(false), dev_valid(false), qrun(0), poisoned(false), qrefs(0), pin_at(0), rec_run(0), rec_w(-1), rec_r(-1) {}
  payload(const payload &o) : std::enable_shared_from_this<payload<P>>(), host(nullptr), dev(nullptr), host_valid(false),
                              dev_valid(false), qrun(0), poisoned(false), qrefs(0), pin_at(0), rec_run(0), rec_w(-1), rec_r(-1) {
    pending();
    o.usable();
    if (o.dev_valid) {  // stays on the device
      check(ctx(), nflhip_memcpy_d2d(ctx(), dev_wo(), o.dev, bytes, ctx_t::queue()), "poly_p copy");
    } else if (o.host_valid) {
      alloc_host();
      std::memcpy(host->data(), o.host->cdata(), bytes);
      host_valid = true;
    }
  }
  payload &operator=(const payload &) = delete;
  ~payload() {
    if (host) {
      host->~P();
      free(host);
    }
    ctx_t::release(dev);
  }
  static nflhip_ctx *ctx() { return ctx_t::get(); }
  static void pending() { lazy<P>::inst().flush(); }  // run whatever is still deferred
  bool queued() const { return qrun != 0 && qrun > lazy<P>::inst().done_run_; }  // (read under the queue's lock, or after pending())
  void usable() const {  // reading a value whose producing operation never ran is an error, not stale HBM
    if (poisoned) throw std::runtime_error("nfl(hip): this polynomial's deferred operation did not run (an earlier operation of its queue failed)");
  }

  void alloc_host() {
    if (host) return;
    void *mem = nullptr;
    if (posix_memalign(&mem, 32, sizeof(P)) != 0) throw std::bad_alloc();
    host = new (mem) P(uninitialized_t());
  }
  // the host image, current
  void to_host() {
    pending();
    usable();
    alloc_host();
    if (host_valid) return;
    if (dev_valid) {
      check(ctx(), nflhip_memcpy_d2h(ctx(), host->data(), dev, bytes, ctx_t::queue()), "poly_p download");
      check(ctx(), nflhip_stream_sync(ctx(), ctx_t::queue()), "poly_p download");
    } else {
      std::memset(static_cast<void *>(host->data()), 0, bytes);
    }
    host_valid = true;
  }
  P &host_rw() {  // the caller may write through the reference: the device image goes stale
    to_host();
    dev_valid = false;
    return *host;
  }
  P const &host_ro() {
    to_host();
    return *host;
  }
  P &host_wo() {  // about to be overwritten entirely on the host
    pending();
    alloc_host();
    host_valid = true;
    dev_valid = false;
    poisoned = false;
    return *host;
  }
  // the device image, current
  const void *dev_ro() {
    pending();
    return dev_ro_nf();
  }
  const void *dev_ro_nf() {  // (the queue's own form: never runs the queue)
    if (queued()) return nullptr;  // produced by a deferred operation; its buffer is assigned when the queue runs (and is the run's until then)
    usable();
    if (!dev) dev = ctx_t::acquire();
    if (!dev_valid) {
      if (host_valid) check(ctx(), nflhip_memcpy_h2d(ctx(), dev, host->cdata(), bytes, ctx_t::queue()), "poly_p upload");
      else check(ctx(), nflhip_memset_dev(ctx(), dev, 0, bytes, ctx_t::queue()), "poly_p zero");
      dev_valid = true;
    }
    return dev;
  }
  void *dev_rw() {  // in-place device operation
    dev_ro();
    host_valid = false;
    return dev;
  }
  void *dev_wo() {  // about to be overwritten entirely on the device
    pending();
    if (!dev) dev = ctx_t::acquire();
    dev_valid = true;
    host_valid = false;
    poisoned = false;
    return dev;
  }
};
}  // namespace detail
}  // namespace nfl
#endif  // NFL_HIP_PAYLOAD_HPP
