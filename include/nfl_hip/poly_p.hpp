// nfl_hip/poly_p.hpp -- part of the drop-in header; include <nfl_hip/nfl.hpp> (or the reference's names under include/nfl*).
// nfl::poly_p (resident handle, copy-on-write, deferred operations).
#ifndef NFL_HIP_POLY_P_HPP
#define NFL_HIP_POLY_P_HPP
#ifndef NFL_HIP_NFL_HPP
#error "include <nfl_hip/nfl.hpp>: the parts depend on each other in its order"
#endif
namespace nfl {
// ---------------------------------------------------------------- poly_p (poly_p.hpp:11-204)
// Copy-on-write handle with the reference's members; the shared payload is RESIDENT (detail::payload): operator
// expressions over handles, transforms, comparisons and the random constructors run on the device and leave the result
// in HBM; poly_obj(), operator()(cm,i), serialisation and the GMP surface bring it to the host (and a non-const access
// marks the device image stale).
template <class T, size_t Degree, size_t NbModuli> class poly_p {
 public:
  typedef poly<T, Degree, NbModuli> poly_type;
  using value_type = typename poly_type::value_type;
  using greater_value_type = typename poly_type::greater_value_type;
  using simd_mode = typename poly_type::simd_mode;
  static constexpr size_t nmoduli = poly_type::nmoduli;
  static constexpr size_t degree = poly_type::degree;
  static constexpr size_t nbits = poly_type::nbits;
  static constexpr size_t aggregated_modulus_bit_size = poly_type::aggregated_modulus_bit_size;

 private:
  typedef detail::payload<poly_type> payload_type;
  typedef typename payload_type::ctx_t ctx_t;
  typedef std::shared_ptr<payload_type> ptr_type;
  mutable ptr_type _p;

  static ptr_type fresh() { return std::allocate_shared<payload_type>(detail::block_pool_alloc<payload_type>()); }
  // constructors: the zero polynomial and the random tags never touch the host; everything else builds the host image
  // with poly's own constructor (same argument meaning, same exceptions)
  static ptr_type make_pointer() { return fresh(); }
  static ptr_type make_pointer(uniform const &m) { ptr_type p = fresh(); sample_into(*p, m); return p; }
  static ptr_type make_pointer(non_uniform const &m) { ptr_type p = fresh(); sample_into(*p, m); return p; }
  static ptr_type make_pointer(ZO_dist const &m) { ptr_type p = fresh(); sample_into(*p, m); return p; }
  static ptr_type make_pointer(hwt_dist const &m) { ptr_type p = fresh(); sample_into(*p, m); return p; }
  template <class in_class, unsigned _lu_depth> static ptr_type make_pointer(gaussian<in_class, T, _lu_depth> const &m) {
    ptr_type p = fresh();
    sample_into(*p, m);
    return p;
  }
  template <class Op, class... A> static ptr_type make_pointer(ops::expr<Op, A...> const &e) {
    ptr_type p = fresh();
    assign_expr(p, e);
    return p;
  }
  // (the overloads above must win over this forwarding template for rvalue tags and expressions)
  template <class X, class Dummy = void> struct device_init : std::false_type {};
  template <class Dummy> struct device_init<uniform, Dummy> : std::true_type {};
  template <class Dummy> struct device_init<non_uniform, Dummy> : std::true_type {};
  template <class Dummy> struct device_init<ZO_dist, Dummy> : std::true_type {};
  template <class Dummy> struct device_init<hwt_dist, Dummy> : std::true_type {};
  template <class in_class, unsigned _lu_depth, class Dummy> struct device_init<gaussian<in_class, T, _lu_depth>, Dummy> : std::true_type {};
  template <class Op, class... A, class Dummy> struct device_init<ops::expr<Op, A...>, Dummy> : std::true_type {};
  template <class A0, class... Args>
  static typename std::enable_if<!device_init<typename std::decay<A0>::type>::value || sizeof...(Args) != 0, ptr_type>::type make_pointer(
      A0 &&a0, Args &&... args) {
    ptr_type p = fresh();
    p->alloc_host();
    p->host->~poly_type();
    new (p->host) poly_type(std::forward<A0>(a0), std::forward<Args>(args)...);
    p->host_valid = true;
    return p;
  }
  // shared with another HANDLE (references held by deferred operations do not count)
  static bool shared(const ptr_type &p, long extra = 0) {
    if (p.use_count() - extra <= 1) return false;  // nobody else at all
    // The queue's reference and the flag that discounts it change together under the queue's lock -- also when a queue
    // run started by ANOTHER thread retires this handle's operations -- so they are read under it.
    std::lock_guard<detail::light_lock> lk(lazy_t::inst().mu);
    return p.use_count() - p->qrefs - extra > 1;
  }
  void detach() const {
    if (shared(_p)) _p = std::allocate_shared<payload_type>(detail::block_pool_alloc<payload_type>(), *_p);  // (device-to-device when the value lives in HBM)
  }
  void detach_for_overwrite() {
    if (shared(_p)) _p = fresh();
  }

  // ---- device-side samplers (same keystream discipline as poly::sample: a fresh stream id per call)
  typedef detail::lazy<poly_type> lazy_t;
  static void check_sample_args(int dist, uint64_t p0, uint64_t p1, const nflhip_gauss *tab) {
    // a deferred constructor must still throw where it is written (core.hpp:205-210): validate with an empty batch
    const unsigned char zero[32] = {0};
    if (tab) detail::check(ctx_t::get(), nflhip_sample_gauss_dev(ctx_t::get(), nullptr, 0, 0, tab, p1, zero, 0, ctx_t::queue()), "set(gaussian)");
    else detail::check(ctx_t::get(), nflhip_sample_dev(ctx_t::get(), nullptr, 0, 0, dist, p0, p1, zero, 0, ctx_t::queue()), "random constructor");
  }
  static bool defer_sample(payload_type &p, int kind, int dist, uint64_t p0, uint64_t p1, uint64_t sid, const nflhip_gauss *tab) {
    if (!lazy_t::usable()) return false;
    if (kind != lazy_t::K_FILL) {
      // (validated once per distinct argument tuple: loops repeat a handful of constructors -- the LWE demo's alternate between two
      //  amplifiers, so remembering only the last one made two validating C-ABI calls per encryption, more than all the recording)
      struct seen_t { int dist; uint64_t p0, p1; const nflhip_gauss *tab; };
      static thread_local seen_t seen[8];
      static thread_local unsigned nseen = 0, victim = 0;
      bool known = false;
      for (unsigned k = 0; k < nseen && !known; ++k)
        known = seen[k].dist == dist && seen[k].p0 == p0 && seen[k].p1 == p1 && seen[k].tab == tab;
      if (!known) {
        check_sample_args(dist, p0, p1, tab);
        const unsigned at = nseen < 8 ? nseen++ : victim++ % 8;
        seen[at] = seen_t{dist, p0, p1, tab};
      }
    }
    lazy_t::inst().record([&](typename lazy_t::op &o) {
      o.kind = static_cast<unsigned char>(kind);
      o.out = &p;
      o.s.dist = dist;
      o.s.p0 = p0;
      o.s.p1 = p1;
      o.s.sid = sid;
      o.s.tab = tab;
    });
    return true;
  }
  static void sample_dist(payload_type &p, int dist, uint64_t p0, uint64_t p1, const char *what) {
    detail::sampler &s = detail::sampler::get();
    const uint64_t sid = s.next++;
    if (defer_sample(p, lazy_t::K_SAMPLE, dist, p0, p1, sid, nullptr)) return;
    detail::check(ctx_t::get(), nflhip_sample_dev(ctx_t::get(), p.dev_wo(), 0, 1, dist, p0, p1, s.key, sid, ctx_t::queue()), what);
  }
  static void sample_into(payload_type &p, uniform const &u) {
    if (u.seeded) {
      if (defer_sample(p, lazy_t::K_FILL, 0, 0, 0, u.seed, nullptr)) return;
      detail::check(ctx_t::get(), nflhip_fill_uniform_dev(ctx_t::get(), p.dev_wo(), 0, 1, u.seed, 0, ctx_t::queue()), "set(uniform)");
    } else {
      sample_dist(p, detail::uniform_rule(), 0, 1, "set(uniform)");
    }
  }
  static void sample_into(payload_type &p, non_uniform const &m) { sample_dist(p, NFLHIP_DIST_BOUNDED, m.upper_bound, m.amplifier, "set(non_uniform)"); }
  static void sample_into(payload_type &p, ZO_dist const &m) { sample_dist(p, NFLHIP_DIST_ZO | detail::dist_flags, m.rho, 1, "set(ZO_dist)"); }
  static void sample_into(payload_type &p, hwt_dist const &m) { sample_dist(p, NFLHIP_DIST_HWT | detail::dist_flags, m.hwt, 1, "set(hwt_dist)"); }
  template <class in_class, unsigned _lu_depth> static void sample_into(payload_type &p, gaussian<in_class, T, _lu_depth> const &m) {
    detail::sampler &s = detail::sampler::get();
    const nflhip_gauss *tab = m.fg_prng->table(ctx_t::get());
    const uint64_t sid = s.next++;
    if (defer_sample(p, lazy_t::K_GAUSS, 0, 0, m.amplifier, sid, tab)) return;
    detail::check(ctx_t::get(), nflhip_sample_gauss_dev(ctx_t::get(), p.dev_wo(), 0, 1, tab, m.amplifier, s.key, sid, ctx_t::queue()),
                  "set(gaussian)");
  }
  // THE evaluation point of an expression tree over handles (core.hpp:24-37): one fused device pass, result resident.
  // `p` is re-seated first when it is shared (copy-on-write without the copy: the whole value is overwritten); the
  // program is lowered BEFORE that, so a tree that reads the old value still sees it.
  template <class Op, class... A> static void assign_expr(ptr_type &p, ops::expr<Op, A...> const &e) {
    ops::program pr;
    e.lower(pr);
    ptr_type keep = p;  // the old payload stays alive while the kernel reads it
    if (shared(p, 1)) p = fresh();  // shared with another handle (`keep` is the extra reference)
    if (ops::expr<Op, A...>::run_resident(pr, *p)) return;
    // through the host: node by node, or trees the fused program cannot hold
    poly_type *tmp = poly_type::make_temp();
    try {
      e.eval(*tmp);
    } catch (...) {
      poly_type::drop_temp(tmp);
      throw;
    }
    std::memcpy(p->host_wo().data(), tmp->cdata(), payload_type::bytes);
    poly_type::drop_temp(tmp);
  }

 public:
  poly_p(poly_p const &o) : _p(o._p) {}
  poly_p(poly_p &o) : _p(const_cast<poly_p const &>(o)._p) {}
  poly_p(poly_p &&o) : _p(std::move(o._p)) {}
  template <class... Args> poly_p(Args &&... args) : _p(make_pointer(std::forward<Args>(args)...)) {}
  poly_p(poly_type const &) = delete;
  poly_p(poly_type &&) = delete;

  // the polynomial as a host object (poly_p.hpp:47-53): forces the value to the host; the non-const form may be
  // written through, so it also retires the device image
  poly_type &poly_obj() {
    detach();
    return _p->host_rw();
  }
  poly_type const &poly_obj() const { return _p->host_ro(); }
  void *payload_id() const { return _p.get(); }  // (engine plumbing: identity of the shared payload)
  bool resident() const { return _p->dev_valid; }  // the current value is in HBM (no upload needed by the next device op)
  // wait for every enqueued operation of this ring type (results are otherwise only awaited when read on the host)
  static void synchronize() {
    lazy_t::inst().flush();
    detail::check(ctx_t::get(), nflhip_stream_sync(ctx_t::get(), ctx_t::queue()), "synchronize");
  }
  // run the deferred operations of this ring type now (without waiting for the device); statistics of the queue so far
  static void flush() { lazy_t::inst().flush(); }
  static size_t deferred_launches() { return lazy_t::inst().launches; }
  static size_t deferred_operations() { return lazy_t::inst().coalesced; }

  template <class Op, class... A> poly_p &operator=(ops::expr<Op, A...> const &e) {
    assign_expr(_p, e);
    return *this;
  }
  poly_p &operator=(uniform const &m) { detach_for_overwrite(); sample_into(*_p, m); return *this; }
  poly_p &operator=(non_uniform const &m) { detach_for_overwrite(); sample_into(*_p, m); return *this; }
  poly_p &operator=(ZO_dist const &m) { detach_for_overwrite(); sample_into(*_p, m); return *this; }
  poly_p &operator=(hwt_dist const &m) { detach_for_overwrite(); sample_into(*_p, m); return *this; }
  template <class in_class, unsigned _lu_depth> poly_p &operator=(gaussian<in_class, T, _lu_depth> const &m) {
    detach_for_overwrite();
    sample_into(*_p, m);
    return *this;
  }
  // (everything else goes through the host polynomial, as in the reference; the overloads above must win for rvalue
  // expressions and tags, which a plain forwarding template would otherwise capture)
  template <class O>
  typename std::enable_if<!device_init<typename std::decay<O>::type>::value && !std::is_same<typename std::decay<O>::type, poly_p>::value,
                          poly_p &>::type
  operator=(O &&o) {
    poly_obj() = std::forward<O>(o);
    return *this;
  }
  poly_p &operator=(std::initializer_list<T> values) {
    poly_obj() = values;
    return *this;
  }
  poly_p &operator=(poly_p const &o) {
    if (this != &o) _p = o._p;
    return *this;
  }
  poly_p &operator=(poly_p &o) { return *this = const_cast<poly_p const &>(o); }
  poly_p &operator=(poly_p &&o) {
    if (this != &o) _p = std::move(o._p);
    return *this;
  }

  bool operator==(poly_p const &o) const { return _p.get() == o._p.get() ? true : bool(ops::make_op<ops::eqmod<T, CC_SIMD>>(*this, o)); }
  bool operator!=(poly_p const &o) const { return _p.get() == o._p.get() ? false : bool(ops::make_op<ops::neqmod<T, CC_SIMD>>(*this, o)); }
  template <class O> bool operator==(O const &o) const { return bool(poly_obj() == o); }
  template <class O> bool operator!=(O const &o) const { return bool(poly_obj() != o); }

  value_type &operator()(size_t cm, size_t i) { return poly_obj()(cm, i); }
  value_type const &operator()(size_t cm, size_t i) const { return poly_obj()(cm, i); }
  template <class M> auto load(size_t cm, size_t i) const -> decltype(M::load(&(this->operator()(cm, i)))) { return M::load(&(*this)(cm, i)); }
  static constexpr value_type get_modulus(size_t n) { return poly_type::get_modulus(n); }

  // Galois automorphism sigma_k (nfl::automorphism / nfl::automorphism_ntt below): the deferred queue of this ring type runs
  // first (on the caller), then one launch on the queue's stream.  The result gets a payload of its own, so `out` may be
  // `in` and copy-on-write sharers of out's old value keep it.
  static void automorphism_into(poly_p &out, poly_p const &in, uint64_t k, int form) {
    lazy_t::inst().flush();
    ptr_type src = in._p;  // (holds the input while the launch is enqueued)
    ptr_type dst = fresh();
    const void *s = src->dev_ro();
    detail::check(ctx_t::get(), nflhip_automorphism_dev(ctx_t::get(), dst->dev_wo(), s, 1, k, form, ctx_t::queue()),
                  form == NFLHIP_FORM_NTT ? "automorphism_ntt" : "automorphism");
    out._p = dst;
  }

  // RNS rescale (nfl::rescale / nfl::rescale_ntt below) into the ring with one modulus less.  That ring type has a deferred
  // queue, a stream and a buffer pool of its own: both queues run first, the output side's stream is awaited (earlier users
  // of the pooled buffer), the launch goes on THIS (the input) side's stream, and the call returns once it has finished
  // there -- operations recorded later on either side see the result.  Never fused into a queue's rewrites.
  template <class, size_t, size_t> friend class poly_p;
  static void rescale_into(poly_p<T, Degree, NbModuli - 1> &out, poly_p const &in, int form) {
    static_assert(NbModuli >= 2, "nfl::rescale drops the last modulus: the input needs at least two");
    typedef poly_p<T, Degree, NbModuli - 1> out_t;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    ptr_type src = in._p;  // (holds the input while the launch is enqueued)
    typename out_t::ptr_type dst = out_t::fresh();
    const void *s = src->dev_ro();
    void *d = dst->dev_wo();
    const char *what = form == NFLHIP_FORM_NTT ? "rescale_ntt" : "rescale";
    detail::check(out_t::ctx_t::get(), nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue()), what);
    detail::check(ctx_t::get(), nflhip_rescale_dev(ctx_t::get(), d, s, 1, form, ctx_t::queue()), what);
    detail::check(ctx_t::get(), nflhip_stream_sync(ctx_t::get(), ctx_t::queue()), what);
    out._p = dst;
  }

  // RNS base conversion and mod-down (nfl::base_convert / nfl::mod_down below).  base_convert works in place on the handle: the
  // deferred queue of this ring type runs first, the value is copied to a payload of its own and converted there on the queue's
  // stream, so copy-on-write sharers of the old value keep it.  mod_down goes into the ring with K moduli less and orders the two
  // ring types' queues and streams exactly as rescale_into does.  Never fused into a queue's rewrites.
  // ntt_form: the NTT-form entries (nfl::base_convert_ntt / nfl::mod_down_ntt), same ordering.
  static void base_convert_into(poly_p &p, size_t s0, size_t ks, size_t d0, size_t kd, bool centered, bool ntt_form = false) {
    lazy_t::inst().flush();
    ptr_type src = p._p;  // (holds the old value while the launches are enqueued)
    ptr_type dst = fresh();
    const void *s = src->dev_ro();
    void *d = dst->dev_wo();
    detail::check(ctx_t::get(), nflhip_memcpy_d2d(ctx_t::get(), d, s, sizeof(T) * Degree * NbModuli, ctx_t::queue()), "base_convert");
    const int flags = centered ? NFLHIP_BASECONV_CENTERED : 0;
    if (ntt_form) detail::check(ctx_t::get(), nflhip_baseconv_ntt_dev(ctx_t::get(), d, d, 1, s0, ks, d0, kd, flags, ctx_t::queue()), "base_convert_ntt");
    else detail::check(ctx_t::get(), nflhip_baseconv_dev(ctx_t::get(), d, d, 1, s0, ks, d0, kd, flags, ctx_t::queue()), "base_convert");
    p._p = dst;
  }
  template <size_t MO> static void mod_down_into(poly_p<T, Degree, MO> &out, poly_p const &in, bool floor, bool ntt_form = false) {
    static_assert(MO >= 1 && MO < NbModuli, "nfl::mod_down drops the last K >= 1 moduli and keeps at least one");
    typedef poly_p<T, Degree, MO> out_t;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    ptr_type src = in._p;  // (holds the input while the launch is enqueued)
    typename out_t::ptr_type dst = out_t::fresh();
    const void *s = src->dev_ro();
    void *d = dst->dev_wo();
    detail::check(out_t::ctx_t::get(), nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue()), "mod_down");
    const int flags = floor ? NFLHIP_MODDOWN_FLOOR : 0;
    if (ntt_form) detail::check(ctx_t::get(), nflhip_moddown_ntt_dev(ctx_t::get(), d, s, 1, NbModuli - MO, flags, ctx_t::queue()), "mod_down_ntt");
    else detail::check(ctx_t::get(), nflhip_moddown_dev(ctx_t::get(), d, s, 1, NbModuli - MO, flags, ctx_t::queue()), "mod_down");
    detail::check(ctx_t::get(), nflhip_stream_sync(ctx_t::get(), ctx_t::queue()), "mod_down");
    out._p = dst;
  }

  // Hybrid key switch (nfl::key_switch_ntt below).  This ring type is the KEY's (NbModuli moduli, the last NbModuli - LO special);
  // in, out0 and out1 live in the ring with LO moduli.  The 2 dnum key polynomials, [term][component], are gathered into one
  // contiguous device buffer of this ring's context.  Both rings' queues run first, the other ring's stream is awaited (the input's
  // pending work, earlier users of the pooled output buffers), the launches go on THIS ring's stream and the call returns once they
  // have finished there -- the ordering of mod_down_into.  The results get payloads of their own: an output may be `in`, and
  // copy-on-write sharers of the outputs' old values keep them.  Never fused into a queue's rewrites.
  template <size_t LO> static void key_switch_into(poly_p<T, Degree, LO> &out0, poly_p<T, Degree, LO> &out1, poly_p<T, Degree, LO> const &in,
                                                   poly_p const *key, size_t alpha, bool centered, bool floor) {
    static_assert(LO >= 1 && LO < NbModuli, "nfl::key_switch_ntt: the key's ring has at least one special modulus more than the input's");
    typedef poly_p<T, Degree, LO> out_t;
    if (alpha == 0 || alpha > LO) throw std::runtime_error("nfl(hip): key_switch_ntt: alpha is out of range (1 to the input's moduli)");
    const size_t dnum = (LO + alpha - 1) / alpha, pb = sizeof(T) * Degree * NbModuli;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename out_t::ptr_type src = in._p;  // (holds the input while the launches are enqueued)
    typename out_t::ptr_type d0 = out_t::fresh(), d1 = out_t::fresh();
    std::vector<ptr_type> held;  // (and the key's payloads)
    for (size_t t = 0; t < 2 * dnum; ++t) held.push_back(key[t]._p);
    const void *s = src->dev_ro();
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo(), *kbuf = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kbuf, 2 * dnum * pb), "key_switch_ntt");
    int rc = NFLHIP_OK;
    for (size_t t = 0; t < 2 * dnum && rc == NFLHIP_OK; ++t)
      rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(kbuf) + t * pb, held[t]->dev_ro(), pb, ctx_t::queue());
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    const int flags = (centered ? NFLHIP_KEYSWITCH_CENTERED : 0) | (floor ? NFLHIP_KEYSWITCH_FLOOR : 0);
    if (rc == NFLHIP_OK) rc = nflhip_keyswitch_ntt_dev(ctx_t::get(), o0, o1, s, kbuf, 1, NbModuli - LO, alpha, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered key goes)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kbuf);
      throw std::runtime_error("nfl(hip): key_switch_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kbuf);
    detail::check(ctx_t::get(), rs, "key_switch_ntt");
    out0._p = d0;
    out1._p = d1;
  }

  // Hoisted rotations (nfl::rotate_hoisted_ntt below).  This ring type is the KEYS' (NbModuli moduli, the last NbModuli - LO special);
  // c0, c1 and the outputs live in the ring with LO moduli.  keys[m] is an array of 2 dnum polynomials, [term][component]; every
  // key is gathered into one contiguous device buffer of this ring's context, key m at polynomial m * 2 dnum.  The ordering is that
  // of key_switch_into: both rings' queues run first, the other ring's stream is awaited, the launches go on THIS ring's stream and
  // the call returns once they have finished there.  The results get payloads of their own: an output may be c0 or c1, and
  // copy-on-write sharers of the outputs' old values keep them.  Never fused into a queue's rewrites.
  template <size_t LO> static void rotate_into(poly_p<T, Degree, LO> *out0s, poly_p<T, Degree, LO> *out1s, poly_p<T, Degree, LO> const *c0,
                                               poly_p<T, Degree, LO> const &c1, poly_p const *const *keys, const uint64_t *ks, size_t count,
                                               size_t alpha, bool centered, bool floor) {
    static_assert(LO >= 1 && LO < NbModuli, "nfl::rotate_hoisted_ntt: the keys' ring has at least one special modulus more than the ciphertext's");
    typedef poly_p<T, Degree, LO> out_t;
    if (alpha == 0 || alpha > LO) throw std::runtime_error("nfl(hip): rotate_hoisted_ntt: alpha is out of range (1 to the ciphertext's moduli)");
    if (count == 0 || count > NFLHIP_ROTATE_MAX_OUTPUTS) throw std::runtime_error("nfl(hip): rotate_hoisted_ntt: 1 to 16 rotations");
    const size_t dnum = (LO + alpha - 1) / alpha, pb = sizeof(T) * Degree * NbModuli, kpolys = 2 * dnum;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename out_t::ptr_type s0 = c0 ? c0->_p : typename out_t::ptr_type(), s1 = c1._p;  // (hold the inputs while the launches are enqueued)
    std::vector<typename out_t::ptr_type> d0, d1;
    std::vector<ptr_type> held;  // (and the keys' payloads)
    void *o0[NFLHIP_ROTATE_MAX_OUTPUTS], *o1[NFLHIP_ROTATE_MAX_OUTPUTS];
    const void *kp[NFLHIP_ROTATE_MAX_OUTPUTS];
    for (size_t m = 0; m < count; ++m) {
      d0.push_back(out_t::fresh());
      d1.push_back(out_t::fresh());
      o0[m] = d0[m]->dev_wo();
      o1[m] = d1[m]->dev_wo();
      for (size_t t = 0; t < kpolys; ++t) held.push_back(keys[m][t]._p);
    }
    const void *p0 = c0 ? s0->dev_ro() : nullptr, *p1 = s1->dev_ro();
    void *kbuf = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kbuf, count * kpolys * pb), "rotate_hoisted_ntt");
    int rc = NFLHIP_OK;
    for (size_t m = 0; m < count; ++m) {
      kp[m] = static_cast<char *>(kbuf) + m * kpolys * pb;
      for (size_t t = 0; t < kpolys && rc == NFLHIP_OK; ++t)
        rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(kbuf) + (m * kpolys + t) * pb, held[m * kpolys + t]->dev_ro(), pb, ctx_t::queue());
    }
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    const int flags = (centered ? NFLHIP_ROTATE_CENTERED : 0) | (floor ? NFLHIP_ROTATE_FLOOR : 0);
    if (rc == NFLHIP_OK) rc = nflhip_rotate_hoisted_ntt_dev(ctx_t::get(), o0, o1, p0, p1, kp, ks, count, 1, NbModuli - LO, alpha, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered keys go)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kbuf);
      throw std::runtime_error("nfl(hip): rotate_hoisted_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kbuf);
    detail::check(ctx_t::get(), rs, "rotate_hoisted_ntt");
    for (size_t m = 0; m < count; ++m) {
      out0s[m]._p = d0[m];
      out1s[m]._p = d1[m];
    }
  }

  // Slot linear transforms (nfl::linear_transform_ntt below).  This ring type is the KEYS' and the diagonals'; c0, c1 and the two
  // outputs live in the ring with LO moduli.  keys[m] is an array of 2 dnum polynomials, [term][component], or NULL for the unrotated
  // diagonal (ks[m] = 1); weights[m] is one polynomial.  Every key and every diagonal is gathered into one contiguous device buffer of
  // this ring's context: term m at polynomial m * (2 dnum + 1), its key first, its diagonal behind it.  The ordering is that of
  // rotate_into.  The results get payloads of their own: an output may be c0 or c1, and copy-on-write sharers of the outputs' old
  // values keep them.  Never fused into a queue's rewrites.
  template <size_t LO> static void linear_transform_into(poly_p<T, Degree, LO> &out0, poly_p<T, Degree, LO> &out1, poly_p<T, Degree, LO> const *c0,
                                                         poly_p<T, Degree, LO> const &c1, poly_p const *const *keys, poly_p const *const *weights,
                                                         const uint64_t *ks, size_t count, size_t alpha, bool centered, bool floor) {
    static_assert(LO >= 1 && LO < NbModuli, "nfl::linear_transform_ntt: the keys' ring has at least one special modulus more than the ciphertext's");
    typedef poly_p<T, Degree, LO> out_t;
    if (alpha == 0 || alpha > LO) throw std::runtime_error("nfl(hip): linear_transform_ntt: alpha is out of range (1 to the ciphertext's moduli)");
    if (count == 0 || count > NFLHIP_LINTRANS_MAX_TERMS) throw std::runtime_error("nfl(hip): linear_transform_ntt: 1 to 16 terms");
    const size_t dnum = (LO + alpha - 1) / alpha, pb = sizeof(T) * Degree * NbModuli, kpolys = 2 * dnum, tpolys = kpolys + 1;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename out_t::ptr_type s0 = c0 ? c0->_p : typename out_t::ptr_type(), s1 = c1._p;  // (hold the inputs while the launches are enqueued)
    typename out_t::ptr_type d0 = out_t::fresh(), d1 = out_t::fresh();
    std::vector<ptr_type> held;  // (and the keys' and the diagonals' payloads: tpolys slots per term, a NULL key's left empty)
    for (size_t m = 0; m < count; ++m) {
      for (size_t t = 0; t < kpolys; ++t) held.push_back(keys[m] ? keys[m][t]._p : ptr_type());
      held.push_back(weights[m]->_p);
    }
    const void *p0 = c0 ? s0->dev_ro() : nullptr, *p1 = s1->dev_ro();
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo();
    void *kbuf = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kbuf, count * tpolys * pb), "linear_transform_ntt");
    const void *kp[NFLHIP_LINTRANS_MAX_TERMS], *wp[NFLHIP_LINTRANS_MAX_TERMS];
    int rc = NFLHIP_OK;
    for (size_t m = 0; m < count; ++m) {
      kp[m] = keys[m] ? static_cast<char *>(kbuf) + m * tpolys * pb : nullptr;
      wp[m] = static_cast<char *>(kbuf) + (m * tpolys + kpolys) * pb;
      for (size_t t = 0; t < tpolys && rc == NFLHIP_OK; ++t)
        if (held[m * tpolys + t])
          rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(kbuf) + (m * tpolys + t) * pb, held[m * tpolys + t]->dev_ro(), pb, ctx_t::queue());
    }
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    const int flags = (centered ? NFLHIP_LINTRANS_CENTERED : 0) | (floor ? NFLHIP_LINTRANS_FLOOR : 0);
    if (rc == NFLHIP_OK) rc = nflhip_lintrans_ntt_dev(ctx_t::get(), o0, o1, p0, p1, kp, wp, ks, count, 1, NbModuli - LO, alpha, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered keys go)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kbuf);
      throw std::runtime_error("nfl(hip): linear_transform_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kbuf);
    detail::check(ctx_t::get(), rs, "linear_transform_ntt");
    out0._p = d0;
    out1._p = d1;
  }

  // Ciphertext multiplication with relinearisation (nfl::mul_relin_ntt / square_relin_ntt / mul_relin_rescale_ntt below).  This ring
  // type is the KEY's (NbModuli moduli, the last NbModuli - LO special); a0, a1, b0, b1 live in the ring with LO moduli (b0 == b1 ==
  // NULL: the square), out0 and out1 in the ring with OO moduli: OO == LO, or OO == LO - 1 for the rescale in the same rounding.  The
  // 2 dnum key polynomials, [term][component], are gathered into one contiguous device buffer of this ring's context.  The ordering is
  // that of key_switch_into, with the outputs' ring type awaited as well.  The results get payloads of their own: an output may be an
  // input, and copy-on-write sharers of the outputs' old values keep them.  Never fused into a queue's rewrites.
  template <size_t LO, size_t OO> static void mul_relin_into(poly_p<T, Degree, OO> &out0, poly_p<T, Degree, OO> &out1, poly_p<T, Degree, LO> const &a0,
                                                             poly_p<T, Degree, LO> const &a1, poly_p<T, Degree, LO> const *b0,
                                                             poly_p<T, Degree, LO> const *b1, poly_p const *key, size_t alpha, bool centered, bool floor) {
    static_assert(LO >= 1 && LO < NbModuli, "nfl::mul_relin_ntt: the key's ring has at least one special modulus more than the ciphertexts'");
    static_assert(OO == LO || OO + 1 == LO, "nfl::mul_relin_ntt: the outputs live in the inputs' ring, or in the ring with one modulus less");
    typedef poly_p<T, Degree, LO> in_t;
    typedef poly_p<T, Degree, OO> out_t;
    if (alpha == 0 || alpha > LO) throw std::runtime_error("nfl(hip): mul_relin_ntt: alpha is out of range (1 to the ciphertexts' moduli)");
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): mul_relin_ntt: b0 and b1 are both given, or both NULL for the square");
    const size_t dnum = (LO + alpha - 1) / alpha, pb = sizeof(T) * Degree * NbModuli;
    lazy_t::inst().flush();
    in_t::lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename in_t::ptr_type s0 = a0._p, s1 = a1._p, t0 = b0 ? b0->_p : typename in_t::ptr_type(), t1 = b1 ? b1->_p : typename in_t::ptr_type();
    typename out_t::ptr_type d0 = out_t::fresh(), d1 = out_t::fresh();
    std::vector<ptr_type> held;  // (the key's payloads)
    for (size_t t = 0; t < 2 * dnum; ++t) held.push_back(key[t]._p);
    const void *p_a0 = s0->dev_ro(), *p_a1 = s1->dev_ro(), *p_b0 = b0 ? t0->dev_ro() : nullptr, *p_b1 = b1 ? t1->dev_ro() : nullptr;
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo(), *kbuf = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kbuf, 2 * dnum * pb), "mul_relin_ntt");
    char *const kb = static_cast<char *>(kbuf);
    int rc = NFLHIP_OK;
    for (size_t t = 0; t < 2 * dnum && rc == NFLHIP_OK; ++t) rc = nflhip_memcpy_d2d(ctx_t::get(), kb + t * pb, held[t]->dev_ro(), pb, ctx_t::queue());
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(in_t::ctx_t::get(), in_t::ctx_t::queue());
    if (rc == NFLHIP_OK && OO != LO) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    const int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0) | (OO != LO ? NFLHIP_MULRELIN_RESCALE : 0);
    if (rc == NFLHIP_OK) rc = nflhip_mulrelin_ntt_dev(ctx_t::get(), o0, o1, p_a0, p_a1, p_b0, p_b1, kbuf, 1, NbModuli - LO, alpha, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered key goes)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kbuf);
      throw std::runtime_error("nfl(hip): mul_relin_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kbuf);
    detail::check(ctx_t::get(), rs, "mul_relin_ntt");
    out0._p = d0;
    out1._p = d1;
  }

  // The two at a level (nfl::key_switch_level_ntt<K> / mul_relin_level_ntt<K> below; include/nflhip.h "leveled key switching").  This
  // ring type is the KEY's: NbModuli moduli, the last K special -- explicit, the types no longer tell.  The operands live in the ring
  // with LO <= NbModuli - K moduli, the level; the outputs of the multiplication in the ring with OO == LO or LO - 1 moduli.  `key` is
  // the ONE top-level key, 2 dnum_L polynomials [term][component]; only the 2 dnum_l LIVE ones, dnum_l = ceil(LO / alpha), are touched
  // and gathered into the device buffer -- whole polynomials of this ring, so that the entry finds phys(r) itself; a live polynomial
  // that is empty (moved from) is refused, a dead one is never looked at.  Ordering, payloads and errors as
  // key_switch_into / mul_relin_into.  Never fused into a queue's rewrites.
  template <size_t K, size_t LO> static void key_switch_level_into(poly_p<T, Degree, LO> &out0, poly_p<T, Degree, LO> &out1,
                                                                   poly_p<T, Degree, LO> const &in, poly_p const *key, size_t alpha, bool centered,
                                                                   bool floor) {
    static_assert(K >= 1 && K < NbModuli && LO >= 1 && LO <= NbModuli - K, "nfl::key_switch_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
    typedef poly_p<T, Degree, LO> out_t;
    if (alpha == 0 || alpha > NbModuli - K) throw std::runtime_error("nfl(hip): key_switch_level_ntt: alpha is out of range (1 to the key ring's ordinary moduli)");
    const size_t live = 2 * ((LO + alpha - 1) / alpha), pb = sizeof(T) * Degree * NbModuli;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename out_t::ptr_type src = in._p;
    typename out_t::ptr_type d0 = out_t::fresh(), d1 = out_t::fresh();
    std::vector<ptr_type> kept;
    for (size_t t = 0; t < live; ++t) {  // (the live polynomials only: the rest of the key may be anything, even moved from)
      if (!key[t]._p) throw std::runtime_error("nfl(hip): a live key polynomial is empty (moved from)");
      kept.push_back(key[t]._p);
    }
    const void *s = src->dev_ro();
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo(), *kgat = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kgat, live * pb), "key_switch_level_ntt");
    int rc = NFLHIP_OK;
    for (size_t t = 0; t < live && rc == NFLHIP_OK; ++t)
      rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(kgat) + t * pb, kept[t]->dev_ro(), pb, ctx_t::queue());
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    int flags = centered ? NFLHIP_KEYSWITCH_CENTERED : 0;
    if (floor) flags |= NFLHIP_KEYSWITCH_FLOOR;
    if (rc == NFLHIP_OK) rc = nflhip_keyswitch_level_ntt_dev(ctx_t::get(), o0, o1, s, kgat, 1, K, alpha, LO, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered key goes)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kgat);
      throw std::runtime_error("nfl(hip): key_switch_level_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kgat);
    detail::check(ctx_t::get(), rs, "key_switch_level_ntt");
    out0._p = d0;
    out1._p = d1;
  }
  template <size_t K, size_t LO, size_t OO> static void mul_relin_level_into(poly_p<T, Degree, OO> &out0, poly_p<T, Degree, OO> &out1,
                                                                             poly_p<T, Degree, LO> const &a0, poly_p<T, Degree, LO> const &a1,
                                                                             poly_p<T, Degree, LO> const *b0, poly_p<T, Degree, LO> const *b1,
                                                                             poly_p const *key, size_t alpha, bool centered, bool floor) {
    static_assert(K >= 1 && K < NbModuli && LO >= 1 && LO <= NbModuli - K, "nfl::mul_relin_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
    static_assert(OO == LO || OO + 1 == LO, "nfl::mul_relin_level_ntt<K>: the outputs live in the inputs' ring, or in the ring with one modulus less");
    typedef poly_p<T, Degree, LO> in_t;
    typedef poly_p<T, Degree, OO> out_t;
    if (alpha == 0 || alpha > NbModuli - K) throw std::runtime_error("nfl(hip): mul_relin_level_ntt: alpha is out of range (1 to the key ring's ordinary moduli)");
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): mul_relin_level_ntt: b0 and b1 are both given, or both NULL for the square");
    const size_t live = 2 * ((LO + alpha - 1) / alpha), pb = sizeof(T) * Degree * NbModuli;
    lazy_t::inst().flush();
    in_t::lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename in_t::ptr_type s0 = a0._p, s1 = a1._p, t0 = b0 ? b0->_p : typename in_t::ptr_type(), t1 = b1 ? b1->_p : typename in_t::ptr_type();
    typename out_t::ptr_type d0 = out_t::fresh(), d1 = out_t::fresh();
    std::vector<ptr_type> kept;
    for (size_t t = 0; t < live; ++t) {  // (the live polynomials only: the rest of the key may be anything, even moved from)
      if (!key[t]._p) throw std::runtime_error("nfl(hip): a live key polynomial is empty (moved from)");
      kept.push_back(key[t]._p);
    }
    const void *p_a0 = s0->dev_ro(), *p_a1 = s1->dev_ro(), *p_b0 = b0 ? t0->dev_ro() : nullptr, *p_b1 = b1 ? t1->dev_ro() : nullptr;
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo(), *kgat = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kgat, live * pb), "mul_relin_level_ntt");
    int rc = NFLHIP_OK;
    for (size_t t = 0; t < live && rc == NFLHIP_OK; ++t)
      rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(kgat) + t * pb, kept[t]->dev_ro(), pb, ctx_t::queue());
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(in_t::ctx_t::get(), in_t::ctx_t::queue());
    if (rc == NFLHIP_OK && OO != LO) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0);
    if (OO != LO) flags |= NFLHIP_MULRELIN_RESCALE;
    if (rc == NFLHIP_OK) rc = nflhip_mulrelin_level_ntt_dev(ctx_t::get(), o0, o1, p_a0, p_a1, p_b0, p_b1, kgat, 1, K, alpha, LO, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered key goes)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kgat);
      throw std::runtime_error("nfl(hip): mul_relin_level_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kgat);
    detail::check(ctx_t::get(), rs, "mul_relin_level_ntt");
    out0._p = d0;
    out1._p = d1;
  }

  // Sums of ciphertext products (nfl::tensor_dot_ntt / mul_relin_dot_level_ntt<K> / square_relin_dot_level_ntt<K> below; include/nflhip.h
  // "sums of ciphertext products").  Every operand is an ARRAY of `terms` polynomials; the arrays are gathered into one device buffer,
  // [operand][term], the way mul_relin_level_into gathers the key, and read as one group of `terms` terms.  tensor_dot_into: this ring
  // type is the operands' and the outputs'.  mul_relin_dot_level_into: this ring type is the KEY's, K and the level LO as in
  // mul_relin_level_into, of which it has the ordering, the payloads and the errors.  Never fused into a queue's rewrites.
  static void tensor_dot_into(poly_p &out0, poly_p &out1, poly_p &out2, poly_p const *a0, poly_p const *a1, poly_p const *b0, poly_p const *b1,
                              size_t terms) {
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): tensor_dot_ntt: b0 and b1 are both given, or both NULL for the squares");
    if (terms == 0) throw std::runtime_error("nfl(hip): tensor_dot_ntt: at least one term");
    const size_t nin = b0 ? 4 : 2, pb = sizeof(T) * Degree * NbModuli;
    lazy_t::inst().flush();
    poly_p const *const ops[4] = {a0, a1, b0, b1};
    std::vector<ptr_type> kept;
    for (size_t k = 0; k < nin; ++k)
      for (size_t j = 0; j < terms; ++j) {
        if (!ops[k][j]._p) throw std::runtime_error("nfl(hip): an operand polynomial is empty (moved from)");
        kept.push_back(ops[k][j]._p);
      }
    ptr_type d0 = fresh(), d1 = fresh(), d2 = fresh();
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo(), *o2 = d2->dev_wo(), *gat = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &gat, nin * terms * pb), "tensor_dot_ntt");
    int rc = NFLHIP_OK;
    for (size_t i = 0; i < kept.size() && rc == NFLHIP_OK; ++i)
      rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(gat) + i * pb, kept[i]->dev_ro(), pb, ctx_t::queue());
    nflhip_dot_operand op[4];
    for (size_t k = 0; k < 4; ++k) op[k].ptr = static_cast<char *>(gat) + (k < nin ? k : 0) * terms * pb, op[k].group_stride = terms, op[k].term_stride = 1;
    if (rc == NFLHIP_OK)
      rc = nflhip_tensor_dot_ntt_dev(ctx_t::get(), o0, o1, o2, &op[0], &op[1], b0 ? &op[2] : nullptr, b0 ? &op[3] : nullptr, 1, terms, NbModuli, 0,
                                     ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered operands go)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), gat);
      throw std::runtime_error("nfl(hip): tensor_dot_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), gat);
    detail::check(ctx_t::get(), rs, "tensor_dot_ntt");
    out0._p = d0;
    out1._p = d1;
    out2._p = d2;
  }
  template <size_t K, size_t LO, size_t OO> static void mul_relin_dot_level_into(poly_p<T, Degree, OO> &out0, poly_p<T, Degree, OO> &out1,
                                                                                 poly_p<T, Degree, LO> const *a0, poly_p<T, Degree, LO> const *a1,
                                                                                 poly_p<T, Degree, LO> const *b0, poly_p<T, Degree, LO> const *b1,
                                                                                 size_t terms, poly_p const *key, size_t alpha, bool centered,
                                                                                 bool floor) {
    static_assert(K >= 1 && K < NbModuli && LO >= 1 && LO <= NbModuli - K, "nfl::mul_relin_dot_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
    static_assert(OO == LO || OO + 1 == LO, "nfl::mul_relin_dot_level_ntt<K>: the outputs live in the inputs' ring, or in the ring with one modulus less");
    typedef poly_p<T, Degree, LO> in_t;
    typedef poly_p<T, Degree, OO> out_t;
    if (alpha == 0 || alpha > NbModuli - K) throw std::runtime_error("nfl(hip): mul_relin_dot_level_ntt: alpha is out of range (1 to the key ring's ordinary moduli)");
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): mul_relin_dot_level_ntt: b0 and b1 are both given, or both NULL for the squares");
    if (terms == 0) throw std::runtime_error("nfl(hip): mul_relin_dot_level_ntt: at least one term");
    const size_t pb = sizeof(T) * Degree * NbModuli, qb = sizeof(T) * Degree * LO, nin = b0 ? 4 : 2, live = 2 * ((LO + alpha - 1) / alpha);
    lazy_t::inst().flush();
    in_t::lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    in_t const *const ops[4] = {a0, a1, b0, b1};
    std::vector<typename in_t::ptr_type> ins;
    for (size_t k = 0; k < nin; ++k)
      for (size_t j = 0; j < terms; ++j) {
        if (!ops[k][j]._p) throw std::runtime_error("nfl(hip): an operand polynomial is empty (moved from)");
        ins.push_back(ops[k][j]._p);
      }
    typename out_t::ptr_type d0 = out_t::fresh(), d1 = out_t::fresh();
    std::vector<ptr_type> kept;
    for (size_t t = 0; t < live; ++t) {  // (the live polynomials only: the rest of the key may be anything, even moved from)
      if (!key[t]._p) throw std::runtime_error("nfl(hip): a live key polynomial is empty (moved from)");
      kept.push_back(key[t]._p);
    }
    std::vector<const void *> src;
    for (size_t i = 0; i < ins.size(); ++i) src.push_back(ins[i]->dev_ro());
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo(), *kgat = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kgat, live * pb + nin * terms * qb), "mul_relin_dot_level_ntt");
    char *const kpos = static_cast<char *>(kgat), *const gat = kpos + live * pb;  // the operands behind the key: [operand][term], LO rows each
    int rc = NFLHIP_OK;
    for (size_t t = 0; t < live && rc == NFLHIP_OK; ++t) rc = nflhip_memcpy_d2d(ctx_t::get(), kpos + t * pb, kept[t]->dev_ro(), pb, ctx_t::queue());
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(in_t::ctx_t::get(), in_t::ctx_t::queue());
    if (rc == NFLHIP_OK && OO != LO) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    for (size_t i = 0; i < src.size() && rc == NFLHIP_OK; ++i) rc = nflhip_memcpy_d2d(ctx_t::get(), gat + i * qb, src[i], qb, ctx_t::queue());
    nflhip_dot_operand op[4];
    for (size_t k = 0; k < 4; ++k) op[k].ptr = gat + (k < nin ? k : 0) * terms * qb, op[k].group_stride = terms, op[k].term_stride = 1;
    int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0);
    if (OO != LO) flags |= NFLHIP_MULRELIN_RESCALE;
    if (rc == NFLHIP_OK)
      rc = nflhip_mulrelin_dot_ntt_dev(ctx_t::get(), o0, o1, &op[0], &op[1], b0 ? &op[2] : nullptr, b0 ? &op[3] : nullptr, kgat, 1, terms, K, alpha, LO, flags,
                                       ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered key and operands go)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kgat);
      throw std::runtime_error("nfl(hip): mul_relin_dot_level_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kgat);
    detail::check(ctx_t::get(), rs, "mul_relin_dot_level_ntt");
    out0._p = d0;
    out1._p = d1;
  }

  // Hoisted rotations and slot linear transforms at a level (nfl::rotate_hoisted_level_ntt<K> / linear_transform_level_ntt<K> below;
  // include/nflhip.h "rotations and linear transforms at a level").  This ring type is the KEYS' and the diagonals': NbModuli moduli,
  // the last K special -- explicit, as in key_switch_level_into.  c0, c1 and the outputs live in the ring with LO <= NbModuli - K
  // moduli, the level.  keys[m] is the ONE top-level Galois key of rotation m, 2 dnum_L polynomials [term][component], of which only
  // the 2 dnum_l LIVE ones, dnum_l = ceil(LO / alpha), are touched and gathered -- whole polynomials of this ring, so that the entry
  // finds phys(r) itself; a live polynomial that is empty (moved from) is refused, a dead one is never looked at.  weights[m] is one
  // whole polynomial of this ring, the top-level diagonal.  Buffer layouts, ordering, payloads and errors as rotate_into /
  // linear_transform_into with dnum_l for dnum.  Never fused into a queue's rewrites.
  template <size_t K, size_t LO> static void rotate_level_into(poly_p<T, Degree, LO> *out0s, poly_p<T, Degree, LO> *out1s,
                                                               poly_p<T, Degree, LO> const *c0, poly_p<T, Degree, LO> const &c1,
                                                               poly_p const *const *keys, const uint64_t *ks, size_t count, size_t alpha,
                                                               bool centered, bool floor) {
    static_assert(K >= 1 && K < NbModuli && LO >= 1 && LO <= NbModuli - K, "nfl::rotate_hoisted_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
    typedef poly_p<T, Degree, LO> out_t;
    if (alpha == 0 || alpha > NbModuli - K) throw std::runtime_error("nfl(hip): rotate_hoisted_level_ntt: alpha is out of range (1 to the key ring's ordinary moduli)");
    if (count == 0 || count > NFLHIP_ROTATE_MAX_OUTPUTS) throw std::runtime_error("nfl(hip): rotate_hoisted_level_ntt: 1 to 16 rotations");
    const size_t rlive = 2 * ((LO + alpha - 1) / alpha), pb = sizeof(T) * Degree * NbModuli;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename out_t::ptr_type s0 = c0 ? c0->_p : typename out_t::ptr_type(), s1 = c1._p;  // (hold the inputs while the launches are enqueued)
    std::vector<typename out_t::ptr_type> d0, d1;
    std::vector<ptr_type> held;  // (and the live key polynomials' payloads)
    void *o0[NFLHIP_ROTATE_MAX_OUTPUTS], *o1[NFLHIP_ROTATE_MAX_OUTPUTS];
    const void *kp[NFLHIP_ROTATE_MAX_OUTPUTS];
    for (size_t m = 0; m < count; ++m) {
      d0.push_back(out_t::fresh());
      d1.push_back(out_t::fresh());
      o0[m] = d0[m]->dev_wo();
      o1[m] = d1[m]->dev_wo();
      for (size_t t = 0; t < rlive; ++t) {
        if (!keys[m][t]._p) throw std::runtime_error("nfl(hip): a live key polynomial is empty (moved from)");
        held.push_back(keys[m][t]._p);
      }
    }
    const void *p0 = c0 ? s0->dev_ro() : nullptr, *p1 = s1->dev_ro();
    void *kgat = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kgat, count * rlive * pb), "rotate_hoisted_level_ntt");
    int rc = NFLHIP_OK;
    for (size_t m = 0; m < count; ++m) {
      kp[m] = static_cast<char *>(kgat) + m * rlive * pb;
      for (size_t t = 0; t < rlive && rc == NFLHIP_OK; ++t)
        rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(kgat) + (m * rlive + t) * pb, held[m * rlive + t]->dev_ro(), pb, ctx_t::queue());
    }
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    const int flags = (centered ? NFLHIP_ROTATE_CENTERED : 0) | (floor ? NFLHIP_ROTATE_FLOOR : 0);
    if (rc == NFLHIP_OK) rc = nflhip_rotate_hoisted_level_ntt_dev(ctx_t::get(), o0, o1, p0, p1, kp, ks, count, 1, K, alpha, LO, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered keys go)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kgat);
      throw std::runtime_error("nfl(hip): rotate_hoisted_level_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kgat);
    detail::check(ctx_t::get(), rs, "rotate_hoisted_level_ntt");
    for (size_t m = 0; m < count; ++m) {
      out0s[m]._p = d0[m];
      out1s[m]._p = d1[m];
    }
  }
  template <size_t K, size_t LO> static void linear_transform_level_into(poly_p<T, Degree, LO> &out0, poly_p<T, Degree, LO> &out1,
                                                                         poly_p<T, Degree, LO> const *c0, poly_p<T, Degree, LO> const &c1,
                                                                         poly_p const *const *keys, poly_p const *const *weights, const uint64_t *ks,
                                                                         size_t count, size_t alpha, bool centered, bool floor) {
    static_assert(K >= 1 && K < NbModuli && LO >= 1 && LO <= NbModuli - K, "nfl::linear_transform_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
    typedef poly_p<T, Degree, LO> out_t;
    if (alpha == 0 || alpha > NbModuli - K) throw std::runtime_error("nfl(hip): linear_transform_level_ntt: alpha is out of range (1 to the key ring's ordinary moduli)");
    if (count == 0 || count > NFLHIP_LINTRANS_MAX_TERMS) throw std::runtime_error("nfl(hip): linear_transform_level_ntt: 1 to 16 terms");
    const size_t tlive = 2 * ((LO + alpha - 1) / alpha), pb = sizeof(T) * Degree * NbModuli, tpolys = tlive + 1;
    const size_t wbytes = pb;  // (a diagonal is a whole polynomial of this ring at every level: the entry reads its rows at phys(r))
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename out_t::ptr_type s0 = c0 ? c0->_p : typename out_t::ptr_type(), s1 = c1._p;  // (hold the inputs while the launches are enqueued)
    typename out_t::ptr_type d0 = out_t::fresh(), d1 = out_t::fresh();
    std::vector<ptr_type> held;  // (the live key polynomials' and the diagonals' payloads: tpolys slots per term, a NULL key's left empty)
    for (size_t m = 0; m < count; ++m) {
      for (size_t t = 0; t < tlive; ++t) {
        if (keys[m] && !keys[m][t]._p) throw std::runtime_error("nfl(hip): a live key polynomial is empty (moved from)");
        held.push_back(keys[m] ? keys[m][t]._p : ptr_type());
      }
      held.push_back(weights[m]->_p);
    }
    const void *p0 = c0 ? s0->dev_ro() : nullptr, *p1 = s1->dev_ro();
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo();
    void *kgat = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kgat, count * tpolys * pb), "linear_transform_level_ntt");
    const void *kp[NFLHIP_LINTRANS_MAX_TERMS], *wp[NFLHIP_LINTRANS_MAX_TERMS];
    int rc = NFLHIP_OK;
    for (size_t m = 0; m < count; ++m) {
      kp[m] = keys[m] ? static_cast<char *>(kgat) + m * tpolys * pb : nullptr;
      wp[m] = static_cast<char *>(kgat) + (m * tpolys + tlive) * pb;
      for (size_t t = 0; t < tpolys && rc == NFLHIP_OK; ++t)
        if (held[m * tpolys + t])
          rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(kgat) + (m * tpolys + t) * pb, held[m * tpolys + t]->dev_ro(),
                                 t < tlive ? pb : wbytes, ctx_t::queue());
    }
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    const int flags = (centered ? NFLHIP_LINTRANS_CENTERED : 0) | (floor ? NFLHIP_LINTRANS_FLOOR : 0);
    if (rc == NFLHIP_OK) rc = nflhip_lintrans_level_ntt_dev(ctx_t::get(), o0, o1, p0, p1, kp, wp, ks, count, 1, K, alpha, LO, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered keys go)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kgat);
      throw std::runtime_error("nfl(hip): linear_transform_level_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kgat);
    detail::check(ctx_t::get(), rs, "linear_transform_level_ntt");
    out0._p = d0;
    out1._p = d1;
  }

  // BSGS slot linear transforms (nfl::bsgs_linear_transform_ntt<K> below; include/nflhip.h "BSGS slot linear transforms").  This ring type
  // is the KEYS' and the diagonals'; the level is the operands' LO.  bkeys[i] / gkeys[j]: the 2 * dnum_L polynomials of a step's top-level
  // Galois key, or NULL for the unrotated step; weights[j * n1 + i]: the top-level diagonal, or NULL for the zero diagonal.  Gathered as
  // linear_transform_level_into gathers: of every key the 2 * dnum_l live polynomials, every diagonal whole; the baby keys first, then
  // the giant keys, then the diagonals.  Never fused into a queue's rewrites.
  template <size_t K, size_t LO> static void bsgs_into(poly_p<T, Degree, LO> &out0, poly_p<T, Degree, LO> &out1, poly_p<T, Degree, LO> const *c0,
                                                       poly_p<T, Degree, LO> const &c1, poly_p const *const *bkeys, const uint64_t *bks, size_t n1,
                                                       poly_p const *const *gkeys, const uint64_t *gks, size_t n2, poly_p const *const *weights,
                                                       size_t alpha, bool centered, bool floor) {
    static_assert(K >= 1 && K < NbModuli && LO >= 1 && LO <= NbModuli - K, "nfl::bsgs_linear_transform_ntt<K>: the level is 1 to the key ring's ordinary moduli");
    typedef poly_p<T, Degree, LO> out_t;
    if (alpha == 0 || alpha > NbModuli - K) throw std::runtime_error("nfl(hip): bsgs_linear_transform_ntt: alpha is out of range (1 to the key ring's ordinary moduli)");
    if (n1 == 0 || n1 > NFLHIP_BSGS_MAX_BABY || n2 == 0 || n2 > NFLHIP_BSGS_MAX_GIANT) throw std::runtime_error("nfl(hip): bsgs_linear_transform_ntt: 1 to 16 baby and giant steps");
    const size_t klive = 2 * ((LO + alpha - 1) / alpha), pb = sizeof(T) * Degree * NbModuli, nkeys = n1 + n2, nw = n1 * n2;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typename out_t::ptr_type s0 = c0 ? c0->_p : typename out_t::ptr_type(), s1 = c1._p;  // (hold the inputs while the launches are enqueued)
    typename out_t::ptr_type d0 = out_t::fresh(), d1 = out_t::fresh();
    std::vector<ptr_type> held;  // (klive slots per key, a NULL key's left empty; then one slot per diagonal, a NULL one's left empty)
    for (size_t m = 0; m < nkeys; ++m) {
      poly_p const *key = m < n1 ? bkeys[m] : gkeys[m - n1];
      for (size_t t = 0; t < klive; ++t) {
        if (key && !key[t]._p) throw std::runtime_error("nfl(hip): a live key polynomial is empty (moved from)");
        held.push_back(key ? key[t]._p : ptr_type());
      }
    }
    for (size_t q = 0; q < nw; ++q) held.push_back(weights[q] ? weights[q]->_p : ptr_type());
    const void *p0 = c0 ? s0->dev_ro() : nullptr, *p1 = s1->dev_ro();
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo();
    void *kgat = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &kgat, held.size() * pb), "bsgs_linear_transform_ntt");
    const void *kp[NFLHIP_BSGS_MAX_BABY + NFLHIP_BSGS_MAX_GIANT], *wp[NFLHIP_BSGS_MAX_BABY * NFLHIP_BSGS_MAX_GIANT];
    int rc = NFLHIP_OK;
    for (size_t t = 0; t < held.size() && rc == NFLHIP_OK; ++t)
      if (held[t]) rc = nflhip_memcpy_d2d(ctx_t::get(), static_cast<char *>(kgat) + t * pb, held[t]->dev_ro(), pb, ctx_t::queue());
    for (size_t m = 0; m < nkeys; ++m) kp[m] = held[m * klive] ? static_cast<char *>(kgat) + m * klive * pb : nullptr;
    for (size_t q = 0; q < nw; ++q) wp[q] = held[nkeys * klive + q] ? static_cast<char *>(kgat) + (nkeys * klive + q) * pb : nullptr;
    if (rc == NFLHIP_OK) rc = nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue());
    const int flags = (centered ? NFLHIP_BSGS_CENTERED : 0) | (floor ? NFLHIP_BSGS_FLOOR : 0);
    if (rc == NFLHIP_OK) rc = nflhip_bsgs_ntt_dev(ctx_t::get(), o0, o1, p0, p1, kp, bks, n1, kp + n1, gks, n2, wp, 1, K, alpha, LO, flags, ctx_t::queue());
    const int rs = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());  // (before the gathered keys go)
    if (rc != NFLHIP_OK) {
      const std::string why = nflhip_last_error(ctx_t::get());  // (before nflhip_free replaces the text)
      nflhip_free(ctx_t::get(), kgat);
      throw std::runtime_error("nfl(hip): bsgs_linear_transform_ntt: " + why);
    }
    nflhip_free(ctx_t::get(), kgat);
    detail::check(ctx_t::get(), rs, "bsgs_linear_transform_ntt");
    out0._p = d0;
    out1._p = d1;
  }

  // The tensor product (nfl::tensor_ntt below): the deferred queue of this ring type runs first, then one launch on its stream.  The
  // results get payloads of their own, so an output may be an input and copy-on-write sharers of the outputs' old values keep them.
  static void tensor_into(poly_p &out0, poly_p &out1, poly_p &out2, poly_p const &a0, poly_p const &a1, poly_p const *b0, poly_p const *b1) {
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): tensor_ntt: b0 and b1 are both given, or both NULL for the square");
    lazy_t::inst().flush();
    ptr_type s0 = a0._p, s1 = a1._p, t0 = b0 ? b0->_p : ptr_type(), t1 = b1 ? b1->_p : ptr_type();
    ptr_type d0 = fresh(), d1 = fresh(), d2 = fresh();
    const void *p_a0 = s0->dev_ro(), *p_a1 = s1->dev_ro(), *p_b0 = b0 ? t0->dev_ro() : nullptr, *p_b1 = b1 ? t1->dev_ro() : nullptr;
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo(), *o2 = d2->dev_wo();
    detail::check(ctx_t::get(), nflhip_tensor_ntt_dev(ctx_t::get(), o0, o1, o2, p_a0, p_a1, p_b0, p_b1, 1, NbModuli, 0, ctx_t::queue()), "tensor_ntt");
    detail::check(ctx_t::get(), nflhip_stream_sync(ctx_t::get(), ctx_t::queue()), "tensor_ntt");
    out0._p = d0;
    out1._p = d1;
    out2._p = d2;
  }

  // Scale-and-round by t/Q (nfl::scale_round / nfl::scale_round_ntt below): this ring type is the input's, out lives in the ring over
  // its first KS moduli, Q their product.  Queues and streams are ordered exactly as mod_down_into orders them.
  template <size_t KS> static void scale_round_into(poly_p<T, Degree, KS> &out, poly_p const &in, uint64_t t, bool floor, bool ntt_form) {
    static_assert(KS >= 1 && KS < NbModuli, "nfl::scale_round: the output's ring is over the first KS moduli, 1 <= KS < the input's");
    typedef poly_p<T, Degree, KS> out_t;
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    ptr_type src = in._p;  // (holds the input while the launch is enqueued)
    typename out_t::ptr_type dst = out_t::fresh();
    const void *s = src->dev_ro();
    void *d = dst->dev_wo();
    detail::check(out_t::ctx_t::get(), nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue()), "scale_round");
    const int flags = floor ? NFLHIP_SCALE_ROUND_FLOOR : 0;
    if (ntt_form) detail::check(ctx_t::get(), nflhip_scale_round_ntt_dev(ctx_t::get(), d, s, 1, KS, t, flags, ctx_t::queue()), "scale_round_ntt");
    else detail::check(ctx_t::get(), nflhip_scale_round_dev(ctx_t::get(), d, s, 1, KS, t, flags, ctx_t::queue()), "scale_round");
    detail::check(ctx_t::get(), nflhip_stream_sync(ctx_t::get(), ctx_t::queue()), "scale_round");
    out._p = dst;
  }

  // The BFV tensor product (nfl::bfv_tensor_ntt below).  This ring type is the EXTENDED one (NbModuli = L + KB moduli); the inputs and
  // the outputs live in the ring with L moduli.  The ordering is that of key_switch_into: both rings' queues run first, the other
  // ring's stream is awaited, the launches go on THIS ring's stream and the call returns once they have finished there.  The results
  // get payloads of their own: an output may be an input.
  template <size_t L> static void bfv_tensor_into(poly_p<T, Degree, L> &out0, poly_p<T, Degree, L> &out1, poly_p<T, Degree, L> &out2,
                                                  poly_p<T, Degree, L> const &a0, poly_p<T, Degree, L> const &a1, poly_p<T, Degree, L> const *b0,
                                                  poly_p<T, Degree, L> const *b1, uint64_t t, bool floor) {
    static_assert(L >= 1 && L < NbModuli, "nfl::bfv_tensor_ntt: the extended ring has at least one modulus more than the ciphertexts'");
    typedef poly_p<T, Degree, L> out_t;
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): bfv_tensor_ntt: b0 and b1 are both given, or both NULL for the square");
    lazy_t::inst().flush();
    out_t::lazy_t::inst().flush();
    typedef typename out_t::ptr_type optr;
    optr s0 = a0._p, s1 = a1._p, t0 = b0 ? b0->_p : optr(), t1 = b1 ? b1->_p : optr();  // (hold the inputs while the launches are enqueued)
    optr d0 = out_t::fresh(), d1 = out_t::fresh(), d2 = out_t::fresh();
    const void *p_a0 = s0->dev_ro(), *p_a1 = s1->dev_ro(), *p_b0 = b0 ? t0->dev_ro() : nullptr, *p_b1 = b1 ? t1->dev_ro() : nullptr;
    void *o0 = d0->dev_wo(), *o1 = d1->dev_wo(), *o2 = d2->dev_wo();
    detail::check(out_t::ctx_t::get(), nflhip_stream_sync(out_t::ctx_t::get(), out_t::ctx_t::queue()), "bfv_tensor_ntt");
    detail::check(ctx_t::get(), nflhip_bfv_tensor_ntt_dev(ctx_t::get(), o0, o1, o2, p_a0, p_a1, p_b0, p_b1, 1, L, t, floor ? NFLHIP_SCALE_ROUND_FLOOR : 0,
                                                          ctx_t::queue()), "bfv_tensor_ntt");
    detail::check(ctx_t::get(), nflhip_stream_sync(ctx_t::get(), ctx_t::queue()), "bfv_tensor_ntt");
    out0._p = d0;
    out1._p = d1;
    out2._p = d2;
  }

  // Sum of products (nfl::dot / nfl::dot_add below): the deferred queue of this ring type runs first (on the caller), then the
  // pointer form of the entry on the queue's stream, 16 terms per launch, chained through the addend.  The result gets a
  // payload of its own, so `out` may be one of the inputs and copy-on-write sharers of out's old value keep it.
  static void dot_into(poly_p &out, poly_p const *a, poly_p const *b, size_t terms, bool add) {
    if (terms == 0) throw std::runtime_error("nfl(hip): dot of zero terms");
    lazy_t::inst().flush();
    ptr_type old = out._p;  // (holds the addend while the launches are enqueued)
    ptr_type dst = fresh();
    void *d = dst->dev_wo();
    const void *addend = add ? old->dev_ro() : nullptr;
    for (size_t k = 0; k < terms; k += NFLHIP_DOT_MAX_POINTERS) {
      const size_t cnt = terms - k < NFLHIP_DOT_MAX_POINTERS ? terms - k : NFLHIP_DOT_MAX_POINTERS;
      ptr_type hold[2 * NFLHIP_DOT_MAX_POINTERS];
      const void *pa[NFLHIP_DOT_MAX_POINTERS], *pb[NFLHIP_DOT_MAX_POINTERS];
      for (size_t j = 0; j < cnt; ++j) {
        hold[2 * j] = a[k + j]._p;
        hold[2 * j + 1] = b[k + j]._p;
        pa[j] = hold[2 * j]->dev_ro();
        pb[j] = hold[2 * j + 1]->dev_ro();
      }
      detail::check(ctx_t::get(), nflhip_dot_ptrs_dev(ctx_t::get(), d, pa, pb, cnt, k == 0 ? addend : d, ctx_t::queue()), "dot");
    }
    out._p = dst;
  }

  // Gadget decomposition (nfl::decompose / nfl::decompose_ntt / nfl::gadget_mul below): the deferred queue of this ring type
  // runs first (on the caller), then ONE launch on the queue's stream writes the dense [terms] block the entry produces into a
  // device buffer of the call, and `terms` device copies hand its polynomials to fresh payloads -- so `in` may be an element of
  // `out` and copy-on-write sharers of out's old values keep them.  The call returns once the stream has drained (the buffer
  // is freed).  flags < 0: gadget_mul.  Never fused into the queue's rewrites.
  static void decompose_into(poly_p *out, poly_p const &in, int w, int flags) {
    const size_t terms = nflhip_decompose_terms(ctx_t::get(), w);
    const char *what = flags < 0 ? "gadget_mul" : "decompose";
    if (terms == 0) throw std::runtime_error(std::string("nfl(hip): ") + what + ": the digit width is out of range");
    lazy_t::inst().flush();
    ptr_type src = in._p;  // (holds the input while the launch is enqueued)
    const void *s = src->dev_ro();
    const size_t one = sizeof(T) * Degree * NbModuli;
    void *block = nullptr;
    detail::check(ctx_t::get(), nflhip_malloc(ctx_t::get(), &block, terms * one), what);
    int rc = flags < 0 ? nflhip_gadget_mul_dev(ctx_t::get(), block, s, 1, w, ctx_t::queue())
                       : nflhip_decompose_dev(ctx_t::get(), block, NFLHIP_FMT_WORDS, s, 1, w, flags, ctx_t::queue());
    std::vector<ptr_type> dst(rc ? 0 : terms);
    try {
      for (size_t j = 0; j < dst.size() && rc == 0; ++j) {
        dst[j] = fresh();
        rc = nflhip_memcpy_d2d(ctx_t::get(), dst[j]->dev_wo(), static_cast<const char *>(block) + j * one, one, ctx_t::queue());
      }
      if (rc == 0) rc = nflhip_stream_sync(ctx_t::get(), ctx_t::queue());
    } catch (...) {
      nflhip_stream_sync(ctx_t::get(), ctx_t::queue());
      nflhip_free(ctx_t::get(), block);
      throw;
    }
    if (rc) nflhip_stream_sync(ctx_t::get(), ctx_t::queue());
    nflhip_free(ctx_t::get(), block);
    detail::check(ctx_t::get(), rc, what);
    for (size_t j = 0; j < terms; ++j) out[j]._p = dst[j];
  }

  /* ntt stuff - public API (poly_p.hpp:141-142): in place in HBM */
  void ntt_pow_phi() { transform(lazy_t::K_NTT_FWD); }
  void invntt_pow_invphi() { transform(lazy_t::K_NTT_INV); }

 private:
  void transform(int kind) {
    bool tried = false;
    if (lazy_t::usable() && !detail::strictmod && _p.use_count() > 1) {
      // queued values carry the queue's reference: the copy-on-write test and the attempt to join the producing record need
      // the queue's lock both -- taken once here instead of twice
      std::lock_guard<detail::light_lock> lk(lazy_t::inst().mu);
      if (_p.use_count() - _p->qrefs <= 1) {
        tried = true;
        if (lazy_t::inst().join_transform(_p.get(), kind)) return;
      }
    }
    detach();
    if (detail::strictmod)
      detail::strict_dev(ctx_t::get(), _p->dev_ro(), 1, ctx_t::queue(), kind == lazy_t::K_NTT_FWD ? "ntt_pow_phi" : "invntt_pow_invphi");
    if (lazy_t::usable()) {
      if (!tried && lazy_t::inst().join_transform(_p.get(), kind)) return;
      lazy_t::inst().record([&](typename lazy_t::op &o) {
        o.kind = static_cast<unsigned char>(kind);
        o.out = _p.get();
      });
      return;
    }
    detail::check(ctx_t::get(), kind == lazy_t::K_NTT_FWD ? nflhip_ntt_fwd_dev(ctx_t::get(), _p->dev_rw(), 1, ctx_t::queue())
                                                          : nflhip_ntt_inv_dev(ctx_t::get(), _p->dev_rw(), 1, ctx_t::queue()),
                  kind == lazy_t::K_NTT_FWD ? "ntt_pow_phi" : "invntt_pow_invphi");
  }

 public:
  void serialize_manually(std::ostream &os) { poly_obj().serialize_manually(os); }
  void deserialize_manually(std::istream &is) { poly_obj().deserialize_manually(is); }
  template <class Archive> void serialize(Archive &archive) { archive(poly_obj()); }

  /* set (poly_p.hpp:161-167) */
  void set(value_type v, bool reduce_coeffs = true) { poly_obj().set(v, reduce_coeffs); }
  void set(uniform const &m) { *this = m; }
  void set(non_uniform const &m) { *this = m; }
  void set(ZO_dist const &m) { *this = m; }
  void set(hwt_dist const &m) { *this = m; }
  template <class in_class, unsigned _lu_depth> void set(gaussian<in_class, T, _lu_depth> const &m) { *this = m; }
  void set(std::initializer_list<value_type> values, bool reduce_coeffs = true) { poly_obj().set(values, reduce_coeffs); }
  void set(std::array<value_type, Degree> values, bool reduce_coeffs = true) { poly_obj().set(values.begin(), values.end(), reduce_coeffs); }
  template <class It> void set(It first, It last, bool reduce_coeffs = true) { poly_obj().set(first, last, reduce_coeffs); }

  /* CRT on limb vectors, as on poly */
  static size_t crt_limbs() { return poly_type::crt_limbs(); }
  void poly2limbs(std::vector<uint64_t> &out) const { poly_obj().poly2limbs(out); }
  void limbs2poly(const uint64_t *limbs, size_t L_in) { poly_obj().limbs2poly(limbs, L_in); }
#ifdef NFL_HIP_WITH_GMP
  /* the GMP-typed surface (poly_p.hpp:186-200) */
  void set_mpz(mpz_t const &v) { poly_obj().set_mpz(v); }
  void set_mpz(std::array<mpz_t, Degree> const &values) { poly_obj().set_mpz(values); }
#ifdef NFL_HIP_HAVE_GMPXX
  void set_mpz(mpz_class const &v) { poly_obj().set_mpz(v); }
  void set_mpz(std::array<mpz_class, Degree> const &values) { poly_obj().set_mpz(values); }
  void set_mpz(std::initializer_list<mpz_class> const &values) { poly_obj().set_mpz(values); }
#endif
  template <class It> void set_mpz(It first, It last) { poly_obj().set_mpz(first, last); }
  std::array<mpz_t, Degree> poly2mpz() { return const_cast<poly_p const *>(this)->poly_obj().poly2mpz(); }
  void poly2mpz(std::array<mpz_t, Degree> &array) { const_cast<poly_p const *>(this)->poly_obj().poly2mpz(array); }
  void mpz2poly(std::array<mpz_t, Degree> const &array) { poly_obj().mpz2poly(array); }
  static size_t bits_in_moduli_product() { return poly_type::bits_in_moduli_product(); }
  static mpz_t &moduli_product() { return poly_type::moduli_product(); }
  static mpz_t &modulus_shoup() { return poly_type::modulus_shoup(); }
  static std::array<mpz_t, nmoduli> lifting_integers() { return poly_type::lifting_integers(); }
#endif
};

template <class T, size_t Degree, size_t AggregatedModulusBitSize>
using poly_p_from_modulus = poly_p<T, Degree, AggregatedModulusBitSize / params<T>::kModulusBitsize>;

template <class T, size_t D, size_t M> std::ostream &operator<<(std::ostream &os, poly_p<T, D, M> const &p) {
  return os << p.poly_obj();
}

/* Galois automorphisms sigma_k : a(X) -> a(X^k) mod (X^n + 1), k odd (include/nflhip.h): coefficient form, and the NTT form
 * ntt_pow_phi() produces.  `out` may be `in`. */
template <class T, size_t D, size_t M> void automorphism(poly<T, D, M> &out, poly<T, D, M> const &in, uint64_t k) {
  typedef poly<T, D, M> P;
  detail::check(P::ctx(), nflhip_automorphism(P::ctx(), out.data(), in.cdata(), 1, k, NFLHIP_FORM_COEFF), "automorphism");
}
template <class T, size_t D, size_t M> void automorphism_ntt(poly<T, D, M> &out, poly<T, D, M> const &in, uint64_t k) {
  typedef poly<T, D, M> P;
  detail::check(P::ctx(), nflhip_automorphism(P::ctx(), out.data(), in.cdata(), 1, k, NFLHIP_FORM_NTT), "automorphism_ntt");
}
template <class T, size_t D, size_t M> void automorphism(poly_p<T, D, M> &out, poly_p<T, D, M> const &in, uint64_t k) {
  poly_p<T, D, M>::automorphism_into(out, in, k, NFLHIP_FORM_COEFF);
}
template <class T, size_t D, size_t M> void automorphism_ntt(poly_p<T, D, M> &out, poly_p<T, D, M> const &in, uint64_t k) {
  poly_p<T, D, M>::automorphism_into(out, in, k, NFLHIP_FORM_NTT);
}

/* RNS rescale (include/nflhip.h): out = round(in / q), q the last modulus of in's ring; out lives in the ring over the first
 * M - 1 moduli.  rescale_ntt takes and leaves values in the order ntt_pow_phi() produces.  M == 1 does not compile. */
template <class T, size_t D, size_t M> void rescale(poly<T, D, M - 1> &out, poly<T, D, M> const &in) {
  static_assert(M >= 2, "nfl::rescale drops the last modulus: the input needs at least two");
  typedef poly<T, D, M> P;
  detail::check(P::ctx(), nflhip_rescale(P::ctx(), out.data(), in.cdata(), 1, NFLHIP_FORM_COEFF), "rescale");
}
template <class T, size_t D, size_t M> void rescale_ntt(poly<T, D, M - 1> &out, poly<T, D, M> const &in) {
  static_assert(M >= 2, "nfl::rescale_ntt drops the last modulus: the input needs at least two");
  typedef poly<T, D, M> P;
  detail::check(P::ctx(), nflhip_rescale(P::ctx(), out.data(), in.cdata(), 1, NFLHIP_FORM_NTT), "rescale_ntt");
}
template <class T, size_t D, size_t M> void rescale(poly_p<T, D, M - 1> &out, poly_p<T, D, M> const &in) {
  poly_p<T, D, M>::rescale_into(out, in, NFLHIP_FORM_COEFF);
}
template <class T, size_t D, size_t M> void rescale_ntt(poly_p<T, D, M - 1> &out, poly_p<T, D, M> const &in) {
  poly_p<T, D, M>::rescale_into(out, in, NFLHIP_FORM_NTT);
}

/* RNS base conversion and mod-down by the last K moduli (include/nflhip.h), coefficient form.  base_convert works in place: rows
 * [d0, d0 + kd) of p become the conversion of rows [s0, s0 + ks), the fast one (x + u Q) or, with centered, the centred
 * representative of x.  mod_down: out = in / P rounded to nearest (floor: floor(in / P) - u), P the product of the last K moduli of
 * in's ring; out lives in the ring over the first M - K moduli, K deduced from the two types. */
template <class T, size_t D, size_t M> void base_convert(poly<T, D, M> &p, size_t s0, size_t ks, size_t d0, size_t kd, bool centered = false) {
  typedef poly<T, D, M> P;
  detail::check(P::ctx(), nflhip_baseconv(P::ctx(), p.data(), p.cdata(), 1, s0, ks, d0, kd, centered ? NFLHIP_BASECONV_CENTERED : 0), "base_convert");
}
template <class T, size_t D, size_t M> void base_convert(poly_p<T, D, M> &p, size_t s0, size_t ks, size_t d0, size_t kd, bool centered = false) {
  poly_p<T, D, M>::base_convert_into(p, s0, ks, d0, kd, centered);
}
template <class T, size_t D, size_t MO, size_t MI> void mod_down(poly<T, D, MO> &out, poly<T, D, MI> const &in, bool floor = false) {
  static_assert(MO >= 1 && MO < MI, "nfl::mod_down drops the last K >= 1 moduli and keeps at least one");
  typedef poly<T, D, MI> P;
  detail::check(P::ctx(), nflhip_moddown(P::ctx(), out.data(), in.cdata(), 1, MI - MO, floor ? NFLHIP_MODDOWN_FLOOR : 0), "mod_down");
}
template <class T, size_t D, size_t MO, size_t MI> void mod_down(poly_p<T, D, MO> &out, poly_p<T, D, MI> const &in, bool floor = false) {
  poly_p<T, D, MI>::template mod_down_into<MO>(out, in, floor);
}

/* The same on NTT-form values (include/nflhip.h "RNS base conversion and mod-down, NTT form"): what base_convert / mod_down make of
 * the coefficient form, forward-transformed -- the mod-up of a digit and the final mod-down of a key switch without leaving the NTT
 * form.  Queues and streams are ordered exactly as by base_convert / mod_down. */
template <class T, size_t D, size_t M> void base_convert_ntt(poly<T, D, M> &p, size_t s0, size_t ks, size_t d0, size_t kd, bool centered = false) {
  typedef poly<T, D, M> P;
  detail::check(P::ctx(), nflhip_baseconv_ntt(P::ctx(), p.data(), p.cdata(), 1, s0, ks, d0, kd, centered ? NFLHIP_BASECONV_CENTERED : 0), "base_convert_ntt");
}
template <class T, size_t D, size_t M> void base_convert_ntt(poly_p<T, D, M> &p, size_t s0, size_t ks, size_t d0, size_t kd, bool centered = false) {
  poly_p<T, D, M>::base_convert_into(p, s0, ks, d0, kd, centered, true);
}
template <class T, size_t D, size_t MO, size_t MI> void mod_down_ntt(poly<T, D, MO> &out, poly<T, D, MI> const &in, bool floor = false) {
  static_assert(MO >= 1 && MO < MI, "nfl::mod_down_ntt drops the last K >= 1 moduli and keeps at least one");
  typedef poly<T, D, MI> P;
  detail::check(P::ctx(), nflhip_moddown_ntt(P::ctx(), out.data(), in.cdata(), 1, MI - MO, floor ? NFLHIP_MODDOWN_FLOOR : 0), "mod_down_ntt");
}
template <class T, size_t D, size_t MO, size_t MI> void mod_down_ntt(poly_p<T, D, MO> &out, poly_p<T, D, MI> const &in, bool floor = false) {
  poly_p<T, D, MI>::template mod_down_into<MO>(out, in, floor, true);
}

/* Hybrid key switching in NTT form (include/nflhip.h "hybrid key switching"): in, out0, out1 in the ring with L moduli, the key in
 * the ring with M > L moduli whose last K = M - L are the special ones; `key` is an array of 2 dnum polynomials in [term][component]
 * order (key[2 d] and key[2 d + 1] belong to digit d), dnum = ceil(L / alpha).  (out0, out1) = the mod-down of sum_d modup(digit d of
 * in) * key[d][c]: one call instead of base_convert_ntt per digit, dot twice and mod_down_ntt twice, with the same words.  An output
 * may be `in`.  On poly the staged host entry; on poly_p the key is gathered into one device buffer and the queues and streams of the
 * two ring types are ordered as nfl::mod_down_ntt orders them. */
template <class T, size_t D, size_t L, size_t M>
void key_switch_ntt(poly<T, D, L> &out0, poly<T, D, L> &out1, poly<T, D, L> const &in, poly<T, D, M> const *key, size_t alpha, bool centered = false,
                    bool floor = false) {
  static_assert(L >= 1 && L < M, "nfl::key_switch_ntt: the key's ring has at least one special modulus more than the input's");
  typedef poly<T, D, L> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  S *t0 = S::make_temp(), *t1 = S::make_temp();  // (an output may be `in`)
  const int flags = (centered ? NFLHIP_KEYSWITCH_CENTERED : 0) | (floor ? NFLHIP_KEYSWITCH_FLOOR : 0);
  const int rc = nflhip_keyswitch_ntt(P::ctx(), t0->data(), t1->data(), in.cdata(), key->cdata(), 1, M - L, alpha, flags);
  if (rc == 0) {
    std::memcpy(static_cast<void *>(out0.data()), t0->cdata(), sizeof(S));
    std::memcpy(static_cast<void *>(out1.data()), t1->cdata(), sizeof(S));
  }
  S::drop_temp(t0);
  S::drop_temp(t1);
  detail::check(P::ctx(), rc, "key_switch_ntt");
}
template <class T, size_t D, size_t L, size_t M>
void key_switch_ntt(poly_p<T, D, L> &out0, poly_p<T, D, L> &out1, poly_p<T, D, L> const &in, poly_p<T, D, M> const *key, size_t alpha,
                    bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template key_switch_into<L>(out0, out1, in, key, alpha, centered, floor);
}

/* Ciphertext multiplication (include/nflhip.h "ciphertext multiplication").  tensor_ntt: (out0, out1, out2) = (a0 b0, a0 b1 + a1 b0,
 * a1 b1) in one pass; an output may be an input.  mul_relin_ntt: the ciphertexts (a0, a1) and (b0, b1) in the ring with L moduli, the
 * key from s^2 to s in the ring with M > L moduli whose last K = M - L are the special ones -- an array of 2 dnum polynomials in
 * [term][component] order, as key_switch_ntt takes it --; (out0, out1) = the tensor product with its third component relinearised,
 * with ONE mod-down: the words of (d0, d1) + key_switch_ntt(d2).  square_relin_ntt: the same of (a0, a1) with itself.
 * mul_relin_rescale_ntt: the outputs live in the ring with L - 1 moduli, divided by the last kept modulus in the same rounding.  An
 * output may be an input.  On poly the staged host entries; on poly_p the key is gathered into one device buffer and the queues
 * and streams of the ring types are ordered as nfl::key_switch_ntt orders them.  Never fused into a queue's rewrites. */
namespace detail {
template <class T, size_t D, size_t L, size_t O, size_t M>
void mul_relin_host(poly<T, D, O> &out0, poly<T, D, O> &out1, poly<T, D, L> const &a0, poly<T, D, L> const &a1, poly<T, D, L> const *b0,
                    poly<T, D, L> const *b1, poly<T, D, M> const *key, size_t alpha, bool centered, bool floor) {
  static_assert(L >= 1 && L < M, "nfl::mul_relin_ntt: the key's ring has at least one special modulus more than the ciphertexts'");
  static_assert(O == L || O + 1 == L, "nfl::mul_relin_ntt: the outputs live in the inputs' ring, or in the ring with one modulus less");
  typedef poly<T, D, O> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  S *t0 = S::make_temp(), *t1 = S::make_temp();  // (an output may be an input)
  const int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0) | (O != L ? NFLHIP_MULRELIN_RESCALE : 0);
  const int rc = nflhip_mulrelin_ntt(P::ctx(), t0->data(), t1->data(), a0.cdata(), a1.cdata(), b0 ? b0->cdata() : nullptr, b1 ? b1->cdata() : nullptr,
                                     key->cdata(), 1, M - L, alpha, flags);
  if (rc == 0) {
    std::memcpy(static_cast<void *>(out0.data()), t0->cdata(), sizeof(S));
    std::memcpy(static_cast<void *>(out1.data()), t1->cdata(), sizeof(S));
  }
  S::drop_temp(t0);
  S::drop_temp(t1);
  check(P::ctx(), rc, "mul_relin_ntt");
}
}  // namespace detail
template <class T, size_t D, size_t M>
void tensor_ntt(poly<T, D, M> &out0, poly<T, D, M> &out1, poly<T, D, M> &out2, poly<T, D, M> const &a0, poly<T, D, M> const &a1,
                poly<T, D, M> const *b0 = nullptr, poly<T, D, M> const *b1 = nullptr) {
  typedef poly<T, D, M> P;
  P *t[3] = {P::make_temp(), P::make_temp(), P::make_temp()};  // (an output may be an input)
  const int rc = nflhip_tensor_ntt(P::ctx(), t[0]->data(), t[1]->data(), t[2]->data(), a0.cdata(), a1.cdata(), b0 ? b0->cdata() : nullptr,
                                   b1 ? b1->cdata() : nullptr, 1, M, 0);
  P *const outs[3] = {&out0, &out1, &out2};
  for (int k = 0; k < 3; ++k) {
    if (rc == 0) std::memcpy(static_cast<void *>(outs[k]->data()), t[k]->cdata(), sizeof(P));
    P::drop_temp(t[k]);
  }
  detail::check(P::ctx(), rc, "tensor_ntt");
}
template <class T, size_t D, size_t M>
void tensor_ntt(poly_p<T, D, M> &out0, poly_p<T, D, M> &out1, poly_p<T, D, M> &out2, poly_p<T, D, M> const &a0, poly_p<T, D, M> const &a1,
                poly_p<T, D, M> const *b0 = nullptr, poly_p<T, D, M> const *b1 = nullptr) {
  poly_p<T, D, M>::tensor_into(out0, out1, out2, a0, a1, b0, b1);
}

/* BFV multiplication (include/nflhip.h "BFV multiplication").  scale_round: out = round(t in / Q) carried back onto the first KS
 * moduli of in's ring, Q their product, KS deduced from the two types (floor: floor(t in / Q) - u); scale_round_ntt: the same on
 * NTT-form values.  bfv_tensor_ntt<KB>: the scale-invariant tensor product of the BFV ciphertexts (a0, a1) and (b0, b1) in the ring
 * with L moduli, through the ring with L + KB moduli: (d0, d1, d2) = round(t (a0 b0, a0 b1 + a1 b0, a1 b1) / Q), NTT form; an output
 * may be an input.  bfv_square_ntt<KB>: the same of (a0, a1) with itself.  The relinearisation is an ordinary key_switch_ntt of d2.  On
 * poly the staged host entries; on poly_p the queues and streams of the two ring types are ordered as nfl::mod_down and
 * nfl::tensor_ntt order theirs.  Never fused into a queue's rewrites. */
template <class T, size_t D, size_t KS, size_t M> void scale_round(poly<T, D, KS> &out, poly<T, D, M> const &in, uint64_t t, bool floor = false) {
  static_assert(KS >= 1 && KS < M, "nfl::scale_round: the output's ring is over the first KS moduli, 1 <= KS < the input's");
  typedef poly<T, D, M> P;
  detail::check(P::ctx(), nflhip_scale_round(P::ctx(), out.data(), in.cdata(), 1, KS, t, floor ? NFLHIP_SCALE_ROUND_FLOOR : 0), "scale_round");
}
template <class T, size_t D, size_t KS, size_t M> void scale_round(poly_p<T, D, KS> &out, poly_p<T, D, M> const &in, uint64_t t, bool floor = false) {
  poly_p<T, D, M>::template scale_round_into<KS>(out, in, t, floor, false);
}
template <class T, size_t D, size_t KS, size_t M> void scale_round_ntt(poly<T, D, KS> &out, poly<T, D, M> const &in, uint64_t t, bool floor = false) {
  static_assert(KS >= 1 && KS < M, "nfl::scale_round_ntt: the output's ring is over the first KS moduli, 1 <= KS < the input's");
  typedef poly<T, D, M> P;
  detail::check(P::ctx(), nflhip_scale_round_ntt(P::ctx(), out.data(), in.cdata(), 1, KS, t, floor ? NFLHIP_SCALE_ROUND_FLOOR : 0), "scale_round_ntt");
}
template <class T, size_t D, size_t KS, size_t M> void scale_round_ntt(poly_p<T, D, KS> &out, poly_p<T, D, M> const &in, uint64_t t, bool floor = false) {
  poly_p<T, D, M>::template scale_round_into<KS>(out, in, t, floor, true);
}
namespace detail {
template <size_t KB, class T, size_t D, size_t L>
void bfv_tensor_host(poly<T, D, L> &out0, poly<T, D, L> &out1, poly<T, D, L> &out2, poly<T, D, L> const &a0, poly<T, D, L> const &a1,
                     poly<T, D, L> const *b0, poly<T, D, L> const *b1, uint64_t t, bool floor) {
  static_assert(KB >= 1, "nfl::bfv_tensor_ntt: the extended ring has at least one modulus more than the ciphertexts'");
  typedef poly<T, D, L> S;
  typedef poly<T, D, L + KB> P;
  S *tmp[3] = {S::make_temp(), S::make_temp(), S::make_temp()};  // (an output may be an input)
  const int rc = nflhip_bfv_tensor_ntt(P::ctx(), tmp[0]->data(), tmp[1]->data(), tmp[2]->data(), a0.cdata(), a1.cdata(), b0 ? b0->cdata() : nullptr,
                                       b1 ? b1->cdata() : nullptr, 1, L, t, floor ? NFLHIP_SCALE_ROUND_FLOOR : 0);
  S *const outs[3] = {&out0, &out1, &out2};
  for (int k = 0; k < 3; ++k) {
    if (rc == 0) std::memcpy(static_cast<void *>(outs[k]->data()), tmp[k]->cdata(), sizeof(S));
    S::drop_temp(tmp[k]);
  }
  check(P::ctx(), rc, "bfv_tensor_ntt");
}
}  // namespace detail
template <size_t KB, class T, size_t D, size_t L>
void bfv_tensor_ntt(poly<T, D, L> &d0, poly<T, D, L> &d1, poly<T, D, L> &d2, poly<T, D, L> const &a0, poly<T, D, L> const &a1, poly<T, D, L> const &b0,
                    poly<T, D, L> const &b1, uint64_t t, bool floor = false) {
  detail::bfv_tensor_host<KB>(d0, d1, d2, a0, a1, &b0, &b1, t, floor);
}
template <size_t KB, class T, size_t D, size_t L>
void bfv_tensor_ntt(poly_p<T, D, L> &d0, poly_p<T, D, L> &d1, poly_p<T, D, L> &d2, poly_p<T, D, L> const &a0, poly_p<T, D, L> const &a1,
                    poly_p<T, D, L> const &b0, poly_p<T, D, L> const &b1, uint64_t t, bool floor = false) {
  poly_p<T, D, L + KB>::template bfv_tensor_into<L>(d0, d1, d2, a0, a1, &b0, &b1, t, floor);
}
template <size_t KB, class T, size_t D, size_t L>
void bfv_square_ntt(poly<T, D, L> &d0, poly<T, D, L> &d1, poly<T, D, L> &d2, poly<T, D, L> const &a0, poly<T, D, L> const &a1, uint64_t t, bool floor = false) {
  detail::bfv_tensor_host<KB, T, D, L>(d0, d1, d2, a0, a1, nullptr, nullptr, t, floor);
}
template <size_t KB, class T, size_t D, size_t L>
void bfv_square_ntt(poly_p<T, D, L> &d0, poly_p<T, D, L> &d1, poly_p<T, D, L> &d2, poly_p<T, D, L> const &a0, poly_p<T, D, L> const &a1, uint64_t t,
                    bool floor = false) {
  poly_p<T, D, L + KB>::template bfv_tensor_into<L>(d0, d1, d2, a0, a1, nullptr, nullptr, t, floor);
}
template <class T, size_t D, size_t L, size_t M>
void mul_relin_ntt(poly<T, D, L> &out0, poly<T, D, L> &out1, poly<T, D, L> const &a0, poly<T, D, L> const &a1, poly<T, D, L> const &b0,
                   poly<T, D, L> const &b1, poly<T, D, M> const *key, size_t alpha, bool centered = false, bool floor = false) {
  detail::mul_relin_host<T, D, L, L, M>(out0, out1, a0, a1, &b0, &b1, key, alpha, centered, floor);
}
template <class T, size_t D, size_t L, size_t M>
void mul_relin_ntt(poly_p<T, D, L> &out0, poly_p<T, D, L> &out1, poly_p<T, D, L> const &a0, poly_p<T, D, L> const &a1, poly_p<T, D, L> const &b0,
                   poly_p<T, D, L> const &b1, poly_p<T, D, M> const *key, size_t alpha, bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template mul_relin_into<L, L>(out0, out1, a0, a1, &b0, &b1, key, alpha, centered, floor);
}
template <class T, size_t D, size_t L, size_t M>
void square_relin_ntt(poly<T, D, L> &out0, poly<T, D, L> &out1, poly<T, D, L> const &a0, poly<T, D, L> const &a1, poly<T, D, M> const *key,
                      size_t alpha, bool centered = false, bool floor = false) {
  detail::mul_relin_host<T, D, L, L, M>(out0, out1, a0, a1, nullptr, nullptr, key, alpha, centered, floor);
}
template <class T, size_t D, size_t L, size_t M>
void square_relin_ntt(poly_p<T, D, L> &out0, poly_p<T, D, L> &out1, poly_p<T, D, L> const &a0, poly_p<T, D, L> const &a1, poly_p<T, D, M> const *key,
                      size_t alpha, bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template mul_relin_into<L, L>(out0, out1, a0, a1, nullptr, nullptr, key, alpha, centered, floor);
}
template <class T, size_t D, size_t L, size_t M>
void mul_relin_rescale_ntt(poly<T, D, L - 1> &out0, poly<T, D, L - 1> &out1, poly<T, D, L> const &a0, poly<T, D, L> const &a1, poly<T, D, L> const &b0,
                           poly<T, D, L> const &b1, poly<T, D, M> const *key, size_t alpha, bool centered = false, bool floor = false) {
  static_assert(L >= 2, "nfl::mul_relin_rescale_ntt drops the last kept modulus: the ciphertexts need at least two");
  detail::mul_relin_host<T, D, L, L - 1, M>(out0, out1, a0, a1, &b0, &b1, key, alpha, centered, floor);
}
template <class T, size_t D, size_t L, size_t M>
void mul_relin_rescale_ntt(poly_p<T, D, L - 1> &out0, poly_p<T, D, L - 1> &out1, poly_p<T, D, L> const &a0, poly_p<T, D, L> const &a1,
                           poly_p<T, D, L> const &b0, poly_p<T, D, L> const &b1, poly_p<T, D, M> const *key, size_t alpha, bool centered = false,
                           bool floor = false) {
  static_assert(L >= 2, "nfl::mul_relin_rescale_ntt drops the last kept modulus: the ciphertexts need at least two");
  poly_p<T, D, M>::template mul_relin_into<L, L - 1>(out0, out1, a0, a1, &b0, &b1, key, alpha, centered, floor);
}

/* The same BELOW the top level (include/nflhip.h "leveled key switching"): x, y0, y1, a*, b* in the ring with Lv moduli, the level; the
 * key is the ONE top-level key in the ring with M moduli whose last K are the special ones, 2 dnum_L polynomials in [term][component]
 * order, dnum_L = ceil((M - K) / alpha).  Lv comes from the types; K cannot be deduced any more, so it is explicit:
 * nfl::key_switch_level_ntt<K>(y0, y1, x, key, alpha).  Lv <= M - K is checked at compile time.  Only the rows [0, Lv) and the K special
 * rows of the first ceil(Lv / alpha) digits of the key are read; on poly_p only those 2 ceil(Lv / alpha) polynomials are gathered.
 * mul_relin_rescale_level_ntt<K>: the outputs live in the ring with Lv - 1 moduli.  Never fused into a queue's rewrites. */
namespace detail {
template <size_t K, class T, size_t D, size_t Lv, size_t O, size_t M>
void mul_relin_level_host(poly<T, D, O> &out0, poly<T, D, O> &out1, poly<T, D, Lv> const &a0, poly<T, D, Lv> const &a1, poly<T, D, Lv> const *b0,
                          poly<T, D, Lv> const *b1, poly<T, D, M> const *key, size_t alpha, bool centered, bool floor) {
  static_assert(K >= 1 && K < M && Lv >= 1 && Lv <= M - K, "nfl::mul_relin_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
  static_assert(O == Lv || O + 1 == Lv, "nfl::mul_relin_level_ntt<K>: the outputs live in the inputs' ring, or in the ring with one modulus less");
  typedef poly<T, D, O> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  S *t0 = S::make_temp(), *t1 = S::make_temp();  // (an output may be an input)
  int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0);
  if (O != Lv) flags |= NFLHIP_MULRELIN_RESCALE;
  const int rc = nflhip_mulrelin_level_ntt(P::ctx(), t0->data(), t1->data(), a0.cdata(), a1.cdata(), b0 ? b0->cdata() : nullptr,
                                           b1 ? b1->cdata() : nullptr, key->cdata(), 1, K, alpha, Lv, flags);
  if (rc == 0) {
    std::memcpy(static_cast<void *>(out0.data()), t0->cdata(), sizeof(S));
    std::memcpy(static_cast<void *>(out1.data()), t1->cdata(), sizeof(S));
  }
  S::drop_temp(t0);
  S::drop_temp(t1);
  check(P::ctx(), rc, "mul_relin_level_ntt");
}
}  // namespace detail
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void key_switch_level_ntt(poly<T, D, Lv> &y0, poly<T, D, Lv> &y1, poly<T, D, Lv> const &x, poly<T, D, M> const *key, size_t alpha, bool centered = false,
                          bool floor = false) {
  static_assert(K >= 1 && K < M && Lv >= 1 && Lv <= M - K, "nfl::key_switch_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
  typedef poly<T, D, Lv> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  S *t0 = S::make_temp(), *t1 = S::make_temp();  // (an output may be `x`)
  int flags = centered ? NFLHIP_KEYSWITCH_CENTERED : 0;
  if (floor) flags |= NFLHIP_KEYSWITCH_FLOOR;
  const int rc = nflhip_keyswitch_level_ntt(P::ctx(), t0->data(), t1->data(), x.cdata(), key->cdata(), 1, K, alpha, Lv, flags);
  if (rc == 0) {
    std::memcpy(static_cast<void *>(y0.data()), t0->cdata(), sizeof(S));
    std::memcpy(static_cast<void *>(y1.data()), t1->cdata(), sizeof(S));
  }
  S::drop_temp(t0);
  S::drop_temp(t1);
  detail::check(P::ctx(), rc, "key_switch_level_ntt");
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void key_switch_level_ntt(poly_p<T, D, Lv> &y0, poly_p<T, D, Lv> &y1, poly_p<T, D, Lv> const &x, poly_p<T, D, M> const *key, size_t alpha,
                          bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template key_switch_level_into<K, Lv>(y0, y1, x, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void mul_relin_level_ntt(poly<T, D, Lv> &out0, poly<T, D, Lv> &out1, poly<T, D, Lv> const &a0, poly<T, D, Lv> const &a1, poly<T, D, Lv> const &b0,
                         poly<T, D, Lv> const &b1, poly<T, D, M> const *key, size_t alpha, bool centered = false, bool floor = false) {
  detail::mul_relin_level_host<K, T, D, Lv, Lv, M>(out0, out1, a0, a1, &b0, &b1, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void mul_relin_level_ntt(poly_p<T, D, Lv> &out0, poly_p<T, D, Lv> &out1, poly_p<T, D, Lv> const &a0, poly_p<T, D, Lv> const &a1,
                         poly_p<T, D, Lv> const &b0, poly_p<T, D, Lv> const &b1, poly_p<T, D, M> const *key, size_t alpha, bool centered = false,
                         bool floor = false) {
  poly_p<T, D, M>::template mul_relin_level_into<K, Lv, Lv>(out0, out1, a0, a1, &b0, &b1, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void square_relin_level_ntt(poly<T, D, Lv> &out0, poly<T, D, Lv> &out1, poly<T, D, Lv> const &a0, poly<T, D, Lv> const &a1, poly<T, D, M> const *key,
                            size_t alpha, bool centered = false, bool floor = false) {
  detail::mul_relin_level_host<K, T, D, Lv, Lv, M>(out0, out1, a0, a1, nullptr, nullptr, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void square_relin_level_ntt(poly_p<T, D, Lv> &out0, poly_p<T, D, Lv> &out1, poly_p<T, D, Lv> const &a0, poly_p<T, D, Lv> const &a1,
                            poly_p<T, D, M> const *key, size_t alpha, bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template mul_relin_level_into<K, Lv, Lv>(out0, out1, a0, a1, nullptr, nullptr, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void mul_relin_rescale_level_ntt(poly<T, D, Lv - 1> &out0, poly<T, D, Lv - 1> &out1, poly<T, D, Lv> const &a0, poly<T, D, Lv> const &a1,
                                 poly<T, D, Lv> const &b0, poly<T, D, Lv> const &b1, poly<T, D, M> const *key, size_t alpha, bool centered = false,
                                 bool floor = false) {
  static_assert(Lv >= 2, "nfl::mul_relin_rescale_level_ntt drops the last live modulus: the level is at least two");
  detail::mul_relin_level_host<K, T, D, Lv, Lv - 1, M>(out0, out1, a0, a1, &b0, &b1, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void mul_relin_rescale_level_ntt(poly_p<T, D, Lv - 1> &out0, poly_p<T, D, Lv - 1> &out1, poly_p<T, D, Lv> const &a0, poly_p<T, D, Lv> const &a1,
                                 poly_p<T, D, Lv> const &b0, poly_p<T, D, Lv> const &b1, poly_p<T, D, M> const *key, size_t alpha,
                                 bool centered = false, bool floor = false) {
  static_assert(Lv >= 2, "nfl::mul_relin_rescale_level_ntt drops the last live modulus: the level is at least two");
  poly_p<T, D, M>::template mul_relin_level_into<K, Lv, Lv - 1>(out0, out1, a0, a1, &b0, &b1, key, alpha, centered, floor);
}

/* Sums of ciphertext products (include/nflhip.h "sums of ciphertext products").  a0, a1, b0, b1 are ARRAYS of `terms` polynomials, term j
 * the ciphertexts (a0[j], a1[j]) and (b0[j], b1[j]).  tensor_dot_ntt: (d0, d1, d2) = sum_j (a0 b0, a0 b1 + a1 b0, a1 b1)(j), in the operands'
 * ring; b0 = b1 = nullptr: the sums of squares.  mul_relin_dot_level_ntt<K>: sum_j ct_a[j] ct_b[j] relinearised ONCE -- the words of
 * (d0, d1) + key_switch_level_ntt<K>(d2) -- with the key, K and the level Lv as in mul_relin_level_ntt<K>; Lv = M - K is the top level.
 * The outputs' ring decides the rescale: poly<T, D, Lv>, or poly<T, D, Lv - 1> for the division by the last live modulus in the same
 * rounding.  square_relin_dot_level_ntt<K>: the sum of squares.  Never fused into a queue's rewrites. */
namespace detail {
template <size_t K, class T, size_t D, size_t Lv, size_t O, size_t M>
void mul_relin_dot_level_host(poly<T, D, O> &out0, poly<T, D, O> &out1, poly<T, D, Lv> const *a0, poly<T, D, Lv> const *a1, poly<T, D, Lv> const *b0,
                              poly<T, D, Lv> const *b1, size_t terms, poly<T, D, M> const *key, size_t alpha, bool centered, bool floor) {
  static_assert(K >= 1 && K < M && Lv >= 1 && Lv <= M - K, "nfl::mul_relin_dot_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
  static_assert(O == Lv || O + 1 == Lv, "nfl::mul_relin_dot_level_ntt<K>: the outputs live in the inputs' ring, or in the ring with one modulus less");
  typedef poly<T, D, O> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T) && sizeof(poly<T, D, Lv>) == D * Lv * sizeof(T), "dense poly arrays");
  S *t0 = S::make_temp(), *t1 = S::make_temp();  // (an output may be an input)
  int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0);
  if (O != Lv) flags |= NFLHIP_MULRELIN_RESCALE;
  const int rc = nflhip_mulrelin_dot_ntt(P::ctx(), t0->data(), t1->data(), a0->cdata(), a1->cdata(), b0 ? b0->cdata() : nullptr, b1 ? b1->cdata() : nullptr,
                                         key->cdata(), 1, terms, 0, K, alpha, Lv, flags);
  if (rc == 0) {
    std::memcpy(static_cast<void *>(out0.data()), t0->cdata(), sizeof(S));
    std::memcpy(static_cast<void *>(out1.data()), t1->cdata(), sizeof(S));
  }
  S::drop_temp(t0);
  S::drop_temp(t1);
  check(P::ctx(), rc, "mul_relin_dot_level_ntt");
}
}  // namespace detail
template <class T, size_t D, size_t M>
void tensor_dot_ntt(poly<T, D, M> &d0, poly<T, D, M> &d1, poly<T, D, M> &d2, poly<T, D, M> const *a0, poly<T, D, M> const *a1, poly<T, D, M> const *b0,
                    poly<T, D, M> const *b1, size_t terms) {
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  P *t[3] = {P::make_temp(), P::make_temp(), P::make_temp()};  // (an output may be an input)
  const int rc = nflhip_tensor_dot_ntt(P::ctx(), t[0]->data(), t[1]->data(), t[2]->data(), a0->cdata(), a1->cdata(), b0 ? b0->cdata() : nullptr,
                                       b1 ? b1->cdata() : nullptr, 1, terms, 0, M, 0);
  P *const outs[3] = {&d0, &d1, &d2};
  for (int k = 0; k < 3; ++k) {
    if (rc == 0) std::memcpy(static_cast<void *>(outs[k]->data()), t[k]->cdata(), sizeof(P));
    P::drop_temp(t[k]);
  }
  detail::check(P::ctx(), rc, "tensor_dot_ntt");
}
template <class T, size_t D, size_t M>
void tensor_dot_ntt(poly_p<T, D, M> &d0, poly_p<T, D, M> &d1, poly_p<T, D, M> &d2, poly_p<T, D, M> const *a0, poly_p<T, D, M> const *a1,
                    poly_p<T, D, M> const *b0, poly_p<T, D, M> const *b1, size_t terms) {
  poly_p<T, D, M>::tensor_dot_into(d0, d1, d2, a0, a1, b0, b1, terms);
}
template <size_t K, class T, size_t D, size_t Lv, size_t O, size_t M>
void mul_relin_dot_level_ntt(poly<T, D, O> &out0, poly<T, D, O> &out1, poly<T, D, Lv> const *a0, poly<T, D, Lv> const *a1, poly<T, D, Lv> const *b0,
                             poly<T, D, Lv> const *b1, size_t terms, poly<T, D, M> const *key, size_t alpha, bool centered = false, bool floor = false) {
  detail::mul_relin_dot_level_host<K, T, D, Lv, O, M>(out0, out1, a0, a1, b0, b1, terms, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t O, size_t M>
void mul_relin_dot_level_ntt(poly_p<T, D, O> &out0, poly_p<T, D, O> &out1, poly_p<T, D, Lv> const *a0, poly_p<T, D, Lv> const *a1,
                             poly_p<T, D, Lv> const *b0, poly_p<T, D, Lv> const *b1, size_t terms, poly_p<T, D, M> const *key, size_t alpha,
                             bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template mul_relin_dot_level_into<K, Lv, O>(out0, out1, a0, a1, b0, b1, terms, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t O, size_t M>
void square_relin_dot_level_ntt(poly<T, D, O> &out0, poly<T, D, O> &out1, poly<T, D, Lv> const *a0, poly<T, D, Lv> const *a1, size_t terms,
                                poly<T, D, M> const *key, size_t alpha, bool centered = false, bool floor = false) {
  detail::mul_relin_dot_level_host<K, T, D, Lv, O, M>(out0, out1, a0, a1, nullptr, nullptr, terms, key, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t O, size_t M>
void square_relin_dot_level_ntt(poly_p<T, D, O> &out0, poly_p<T, D, O> &out1, poly_p<T, D, Lv> const *a0, poly_p<T, D, Lv> const *a1, size_t terms,
                                poly_p<T, D, M> const *key, size_t alpha, bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template mul_relin_dot_level_into<K, Lv, O>(out0, out1, a0, a1, static_cast<poly_p<T, D, Lv> const *>(nullptr),
                                                                static_cast<poly_p<T, D, Lv> const *>(nullptr), terms, key, alpha, centered, floor);
}

/* Hoisted rotations (include/nflhip.h "hoisted rotations"): the ciphertext (c0, c1) in the ring with L moduli rotated by ks[m], m <
 * count <= 16, against keys[m] -- an array of 2 dnum polynomials in [term][component] order, dnum = ceil(L / alpha), in the ring with
 * M > L moduli whose last K = M - L are the special ones (K is deduced from the types, as in key_switch_ntt).  For every m
 * (out0s[m], out1s[m]) = sigma^NTT_ks[m] of (key_switch_ntt(c1, keys[m]) + (c0, 0)): one mod-up of c1 serves every rotation.  keys[m]
 * switches from s to sigma_(ks[m]^-1)(s): the usual Galois key for ks[m] with automorphism_ntt by ks[m]^-1 applied to every polynomial.
 * c0 may be NULL; an output may be c0 or c1.  On poly the staged host entry; on poly_p the keys are gathered into one device buffer
 * and the queues and streams of the two ring types are ordered as nfl::key_switch_ntt orders them. */
template <class T, size_t D, size_t L, size_t M>
void rotate_hoisted_ntt(poly<T, D, L> *out0s, poly<T, D, L> *out1s, poly<T, D, L> const *c0, poly<T, D, L> const &c1, poly<T, D, M> const *const *keys,
                        const uint64_t *ks, size_t count, size_t alpha, bool centered = false, bool floor = false) {
  static_assert(L >= 1 && L < M, "nfl::rotate_hoisted_ntt: the keys' ring has at least one special modulus more than the ciphertext's");
  typedef poly<T, D, L> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  if (count == 0 || count > NFLHIP_ROTATE_MAX_OUTPUTS) throw std::runtime_error("nfl(hip): rotate_hoisted_ntt: 1 to 16 rotations");
  S *t0[NFLHIP_ROTATE_MAX_OUTPUTS], *t1[NFLHIP_ROTATE_MAX_OUTPUTS];  // (an output may be an input)
  void *o0[NFLHIP_ROTATE_MAX_OUTPUTS], *o1[NFLHIP_ROTATE_MAX_OUTPUTS];
  const void *kp[NFLHIP_ROTATE_MAX_OUTPUTS];
  for (size_t m = 0; m < count; ++m) {
    t0[m] = S::make_temp();
    t1[m] = S::make_temp();
    o0[m] = t0[m]->data();
    o1[m] = t1[m]->data();
    kp[m] = keys[m]->cdata();
  }
  const int flags = (centered ? NFLHIP_ROTATE_CENTERED : 0) | (floor ? NFLHIP_ROTATE_FLOOR : 0);
  const int rc = nflhip_rotate_hoisted_ntt(P::ctx(), o0, o1, c0 ? c0->cdata() : nullptr, c1.cdata(), kp, ks, count, 1, M - L, alpha, flags);
  for (size_t m = 0; m < count; ++m) {
    if (rc == 0) {
      std::memcpy(static_cast<void *>(out0s[m].data()), t0[m]->cdata(), sizeof(S));
      std::memcpy(static_cast<void *>(out1s[m].data()), t1[m]->cdata(), sizeof(S));
    }
    S::drop_temp(t0[m]);
    S::drop_temp(t1[m]);
  }
  detail::check(P::ctx(), rc, "rotate_hoisted_ntt");
}
template <class T, size_t D, size_t L, size_t M>
void rotate_hoisted_ntt(poly_p<T, D, L> *out0s, poly_p<T, D, L> *out1s, poly_p<T, D, L> const *c0, poly_p<T, D, L> const &c1,
                        poly_p<T, D, M> const *const *keys, const uint64_t *ks, size_t count, size_t alpha, bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template rotate_into<L>(out0s, out1s, c0, c1, keys, ks, count, alpha, centered, floor);
}

/* Slot linear transforms (include/nflhip.h "slot linear transforms"): (out0, out1) = sum_m weights[m] * sigma_ks[m](c0, c1) for m < count
 * <= 16 with ONE mod-down: the key-switch sums of c1 against keys[m] are permuted, multiplied by the diagonals and added up on all M
 * rows, then modded down once; the c0 terms and the unrotated diagonals are added on the L rows.  keys[m] as for rotate_hoisted_ntt, or
 * NULL for the unrotated diagonal (ks[m] = 1 mod 2 D); weights[m] one polynomial of the ring with M moduli, the diagonal in NTT form.
 * Not the words of a weighted sum of rotate_hoisted_ntt results: one rounding instead of `count`.  c0 may be NULL; an output may be c0
 * or c1.  On poly the staged host entry, the outputs through temporaries; on poly_p the ordering of rotate_hoisted_ntt. */
template <class T, size_t D, size_t L, size_t M>
void linear_transform_ntt(poly<T, D, L> &out0, poly<T, D, L> &out1, poly<T, D, L> const *c0, poly<T, D, L> const &c1, poly<T, D, M> const *const *keys,
                          poly<T, D, M> const *const *weights, const uint64_t *ks, size_t count, size_t alpha, bool centered = false,
                          bool floor = false) {
  static_assert(L >= 1 && L < M, "nfl::linear_transform_ntt: the keys' ring has at least one special modulus more than the ciphertext's");
  typedef poly<T, D, L> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  if (count == 0 || count > NFLHIP_LINTRANS_MAX_TERMS) throw std::runtime_error("nfl(hip): linear_transform_ntt: 1 to 16 terms");
  const void *kp[NFLHIP_LINTRANS_MAX_TERMS], *wp[NFLHIP_LINTRANS_MAX_TERMS];
  for (size_t m = 0; m < count; ++m) {
    kp[m] = keys[m] ? keys[m]->cdata() : nullptr;
    wp[m] = weights[m]->cdata();
  }
  S *t0 = S::make_temp(), *t1 = S::make_temp();  // (an output may be an input)
  const int flags = (centered ? NFLHIP_LINTRANS_CENTERED : 0) | (floor ? NFLHIP_LINTRANS_FLOOR : 0);
  const int rc = nflhip_lintrans_ntt(P::ctx(), t0->data(), t1->data(), c0 ? c0->cdata() : nullptr, c1.cdata(), kp, wp, ks, count, 1, M - L, alpha, flags);
  if (rc == 0) {
    std::memcpy(static_cast<void *>(out0.data()), t0->cdata(), sizeof(S));
    std::memcpy(static_cast<void *>(out1.data()), t1->cdata(), sizeof(S));
  }
  S::drop_temp(t0);
  S::drop_temp(t1);
  detail::check(P::ctx(), rc, "linear_transform_ntt");
}
template <class T, size_t D, size_t L, size_t M>
void linear_transform_ntt(poly_p<T, D, L> &out0, poly_p<T, D, L> &out1, poly_p<T, D, L> const *c0, poly_p<T, D, L> const &c1,
                          poly_p<T, D, M> const *const *keys, poly_p<T, D, M> const *const *weights, const uint64_t *ks, size_t count, size_t alpha,
                          bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template linear_transform_into<L>(out0, out1, c0, c1, keys, weights, ks, count, alpha, centered, floor);
}

/* The two BELOW the top level (include/nflhip.h "rotations and linear transforms at a level"): c0, c1 and the outputs in the ring with Lv
 * moduli, the level; keys[m] the ONE top-level Galois key of rotation m in the ring with M moduli whose last K are the special ones,
 * 2 dnum_L polynomials in [term][component] order (the first 2 ceil(Lv / alpha) are read), or NULL for the unrotated diagonal of a
 * linear transform; weights[m] the ONE top-level diagonal, a polynomial of the ring with M moduli.  K cannot be deduced from the types
 * any more and is the explicit template argument: nfl::rotate_hoisted_level_ntt<K>(out0s, out1s, c0, c1, keys, ks, count, alpha).
 * Lv <= M - K is checked at compile time.  Only the rows [0, Lv) and the K special rows of the keys and diagonals are read.  Never
 * fused into a queue's rewrites. */
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void rotate_hoisted_level_ntt(poly<T, D, Lv> *out0s, poly<T, D, Lv> *out1s, poly<T, D, Lv> const *c0, poly<T, D, Lv> const &c1,
                              poly<T, D, M> const *const *keys, const uint64_t *ks, size_t count, size_t alpha, bool centered = false,
                              bool floor = false) {
  static_assert(K >= 1 && K < M && Lv >= 1 && Lv <= M - K, "nfl::rotate_hoisted_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
  typedef poly<T, D, Lv> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  if (count == 0 || count > NFLHIP_ROTATE_MAX_OUTPUTS) throw std::runtime_error("nfl(hip): rotate_hoisted_level_ntt: 1 to 16 rotations");
  S *t0[NFLHIP_ROTATE_MAX_OUTPUTS], *t1[NFLHIP_ROTATE_MAX_OUTPUTS];  // (an output may be an input)
  void *o0[NFLHIP_ROTATE_MAX_OUTPUTS], *o1[NFLHIP_ROTATE_MAX_OUTPUTS];
  const void *kp[NFLHIP_ROTATE_MAX_OUTPUTS];
  for (size_t m = 0; m < count; ++m) {
    t0[m] = S::make_temp();
    t1[m] = S::make_temp();
    o0[m] = t0[m]->data();
    o1[m] = t1[m]->data();
    kp[m] = (*keys[m]).cdata();
  }
  const int flags = (centered ? NFLHIP_ROTATE_CENTERED : 0) | (floor ? NFLHIP_ROTATE_FLOOR : 0);
  const int rc = nflhip_rotate_hoisted_level_ntt(P::ctx(), o0, o1, c0 ? c0->cdata() : nullptr, c1.cdata(), kp, ks, count, 1, K, alpha, Lv, flags);
  for (size_t m = 0; m < count; ++m) {
    if (rc == 0) {
      std::memcpy(static_cast<void *>(out0s[m].data()), t0[m]->cdata(), sizeof(S));
      std::memcpy(static_cast<void *>(out1s[m].data()), t1[m]->cdata(), sizeof(S));
    }
    S::drop_temp(t0[m]);
    S::drop_temp(t1[m]);
  }
  detail::check(P::ctx(), rc, "rotate_hoisted_level_ntt");
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void rotate_hoisted_level_ntt(poly_p<T, D, Lv> *out0s, poly_p<T, D, Lv> *out1s, poly_p<T, D, Lv> const *c0, poly_p<T, D, Lv> const &c1,
                              poly_p<T, D, M> const *const *keys, const uint64_t *ks, size_t count, size_t alpha, bool centered = false,
                              bool floor = false) {
  poly_p<T, D, M>::template rotate_level_into<K, Lv>(out0s, out1s, c0, c1, keys, ks, count, alpha, centered, floor);
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void linear_transform_level_ntt(poly<T, D, Lv> &out0, poly<T, D, Lv> &out1, poly<T, D, Lv> const *c0, poly<T, D, Lv> const &c1,
                                poly<T, D, M> const *const *keys, poly<T, D, M> const *const *weights, const uint64_t *ks, size_t count, size_t alpha,
                                bool centered = false, bool floor = false) {
  static_assert(K >= 1 && K < M && Lv >= 1 && Lv <= M - K, "nfl::linear_transform_level_ntt<K>: the level is 1 to the key ring's ordinary moduli");
  typedef poly<T, D, Lv> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  if (count == 0 || count > NFLHIP_LINTRANS_MAX_TERMS) throw std::runtime_error("nfl(hip): linear_transform_level_ntt: 1 to 16 terms");
  const void *kp[NFLHIP_LINTRANS_MAX_TERMS], *wp[NFLHIP_LINTRANS_MAX_TERMS];
  for (size_t m = 0; m < count; ++m) {
    kp[m] = keys[m] ? keys[m]->cdata() : nullptr;
    wp[m] = weights[m]->cdata();
  }
  S *t0 = S::make_temp(), *t1 = S::make_temp();  // (an output may be an input)
  const int flags = (centered ? NFLHIP_LINTRANS_CENTERED : 0) | (floor ? NFLHIP_LINTRANS_FLOOR : 0);
  const int rc = nflhip_lintrans_level_ntt(P::ctx(), t0->data(), t1->data(), c0 ? c0->cdata() : nullptr, c1.cdata(), kp, wp, ks, count, 1, K, alpha, Lv,
                                           flags);
  if (rc == 0) {
    std::memcpy(static_cast<void *>(out0.data()), t0->cdata(), sizeof(S));
    std::memcpy(static_cast<void *>(out1.data()), t1->cdata(), sizeof(S));
  }
  S::drop_temp(t0);
  S::drop_temp(t1);
  detail::check(P::ctx(), rc, "linear_transform_level_ntt");
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void linear_transform_level_ntt(poly_p<T, D, Lv> &out0, poly_p<T, D, Lv> &out1, poly_p<T, D, Lv> const *c0, poly_p<T, D, Lv> const &c1,
                                poly_p<T, D, M> const *const *keys, poly_p<T, D, M> const *const *weights, const uint64_t *ks, size_t count,
                                size_t alpha, bool centered = false, bool floor = false) {
  poly_p<T, D, M>::template linear_transform_level_into<K, Lv>(out0, out1, c0, c1, keys, weights, ks, count, alpha, centered, floor);
}

/* BSGS slot linear transforms (include/nflhip.h "BSGS slot linear transforms"): sum_j sigma_{gks[j]}(sum_i weights[j * n1 + i] (.)
 * sigma_{bks[i]}(c0, c1)) in one call with ONE mod-down of two polynomials.  The level comes from the operand types (Lv = M - K is the
 * top); bkeys[i] / gkeys[j] point to the 2 * dnum_L polynomials of a step's top-level Galois key, or are NULL for the unrotated step
 * (k = 1); weights[j * n1 + i] points to the top-level diagonal, or is NULL for the zero diagonal.  c0 may be NULL; an output may be an
 * input.  On poly through the staged host entry; on poly_p on the resident values, gathered as linear_transform_level_ntt gathers. */
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void bsgs_linear_transform_ntt(poly<T, D, Lv> &out0, poly<T, D, Lv> &out1, poly<T, D, Lv> const *c0, poly<T, D, Lv> const &c1,
                               poly<T, D, M> const *const *bkeys, const uint64_t *bks, size_t n1, poly<T, D, M> const *const *gkeys, const uint64_t *gks,
                               size_t n2, poly<T, D, M> const *const *weights, size_t alpha, bool centered = false, bool floor = false) {
  static_assert(K >= 1 && K < M && Lv >= 1 && Lv <= M - K, "nfl::bsgs_linear_transform_ntt<K>: the level is 1 to the key ring's ordinary moduli");
  typedef poly<T, D, Lv> S;
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  if (n1 == 0 || n1 > NFLHIP_BSGS_MAX_BABY || n2 == 0 || n2 > NFLHIP_BSGS_MAX_GIANT) throw std::runtime_error("nfl(hip): bsgs_linear_transform_ntt: 1 to 16 baby and giant steps");
  const void *bp[NFLHIP_BSGS_MAX_BABY], *gp[NFLHIP_BSGS_MAX_GIANT], *wp[NFLHIP_BSGS_MAX_BABY * NFLHIP_BSGS_MAX_GIANT];
  for (size_t i = 0; i < n1; ++i) bp[i] = bkeys[i] ? bkeys[i]->cdata() : nullptr;
  for (size_t j = 0; j < n2; ++j) gp[j] = gkeys[j] ? gkeys[j]->cdata() : nullptr;
  for (size_t q = 0; q < n1 * n2; ++q) wp[q] = weights[q] ? weights[q]->cdata() : nullptr;
  S *t0 = S::make_temp(), *t1 = S::make_temp();  // (an output may be an input)
  const int flags = (centered ? NFLHIP_BSGS_CENTERED : 0) | (floor ? NFLHIP_BSGS_FLOOR : 0);
  const int rc = nflhip_bsgs_ntt(P::ctx(), t0->data(), t1->data(), c0 ? c0->cdata() : nullptr, c1.cdata(), bp, bks, n1, gp, gks, n2, wp, 1, K, alpha, Lv,
                                 flags);
  if (rc == 0) {
    std::memcpy(static_cast<void *>(out0.data()), t0->cdata(), sizeof(S));
    std::memcpy(static_cast<void *>(out1.data()), t1->cdata(), sizeof(S));
  }
  S::drop_temp(t0);
  S::drop_temp(t1);
  detail::check(P::ctx(), rc, "bsgs_linear_transform_ntt");
}
template <size_t K, class T, size_t D, size_t Lv, size_t M>
void bsgs_linear_transform_ntt(poly_p<T, D, Lv> &out0, poly_p<T, D, Lv> &out1, poly_p<T, D, Lv> const *c0, poly_p<T, D, Lv> const &c1,
                               poly_p<T, D, M> const *const *bkeys, const uint64_t *bks, size_t n1, poly_p<T, D, M> const *const *gkeys,
                               const uint64_t *gks, size_t n2, poly_p<T, D, M> const *const *weights, size_t alpha, bool centered = false,
                               bool floor = false) {
  poly_p<T, D, M>::template bsgs_into<K, Lv>(out0, out1, c0, c1, bkeys, bks, n1, gkeys, gks, n2, weights, alpha, centered, floor);
}

/* Sums of products across polynomials (include/nflhip.h): out = sum_{j < terms} a[j] * b[j], element-wise in every row -- the
 * inner product of NTT-form operands.  dot_add: out += the sum.  a and b are arrays of `terms` polynomials; out may be one of
 * them.  On poly the arrays go through the staged host entry; on poly_p the sum runs on the resident values. */
template <class T, size_t D, size_t M> void dot(poly<T, D, M> &out, poly<T, D, M> const *a, poly<T, D, M> const *b, size_t terms) {
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  P *tmp = P::make_temp();  // (out may be an element of a or b)
  const int rc = nflhip_dot(P::ctx(), tmp->data(), a->cdata(), b->cdata(), 1, terms, 0);
  if (rc == 0) std::memcpy(static_cast<void *>(out.data()), tmp->cdata(), sizeof(P));
  P::drop_temp(tmp);
  detail::check(P::ctx(), rc, "dot");
}
template <class T, size_t D, size_t M> void dot_add(poly<T, D, M> &out, poly<T, D, M> const *a, poly<T, D, M> const *b, size_t terms) {
  typedef poly<T, D, M> P;
  P *tmp = P::make_temp();
  try {
    dot(*tmp, a, b, terms);
    out = out + *tmp;
  } catch (...) {
    P::drop_temp(tmp);
    throw;
  }
  P::drop_temp(tmp);
}
template <class T, size_t D, size_t M> void dot(poly_p<T, D, M> &out, poly_p<T, D, M> const *a, poly_p<T, D, M> const *b, size_t terms) {
  poly_p<T, D, M>::dot_into(out, a, b, terms, false);
}
template <class T, size_t D, size_t M> void dot_add(poly_p<T, D, M> &out, poly_p<T, D, M> const *a, poly_p<T, D, M> const *b, size_t terms) {
  poly_p<T, D, M>::dot_into(out, a, b, terms, true);
}

/* Gadget decomposition (include/nflhip.h): the base-2^w digits of every row of a COEFFICIENT-form polynomial.  `out` is an array of
 * gadget_terms<P>(w) = nmoduli * ceil(modulus bits / w) polynomials of the same ring type: out[m * l + t] holds digit t of row m,
 * spread over every row (balanced digits in [-B/2, B/2] with signed_digits).  decompose_ntt leaves the digit polynomials in the
 * order ntt_pow_phi() produces.  gadget_mul is the key-generation companion: out[m * l + t] = in * 2^(w t) in row m, zero in the
 * other rows, so that  sum_j decompose(x)[j] * gadget_mul(y)[j] = x * y  in every row (nfl::dot over NTT-form operands).
 * `in` may be an element of `out`.  On poly the call goes through the staged host entry (gadget_mul: a device buffer of the
 * call); on poly_p it runs on the resident value. */
template <class P> inline size_t gadget_terms(int w) {
  const int bits = int(8 * sizeof(typename P::value_type)) - 2;
  return w < 1 || w > bits - 1 ? 0 : P::nmoduli * size_t((bits + w - 1) / w);
}
namespace detail {
template <class T, size_t D, size_t M> void decompose_host(poly<T, D, M> *out, poly<T, D, M> const &in, int w, int flags) {
  typedef poly<T, D, M> P;
  static_assert(sizeof(P) == D * M * sizeof(T), "dense poly array");
  const size_t terms = gadget_terms<P>(w);
  const char *what = flags < 0 ? "gadget_mul" : "decompose";
  if (terms == 0) throw std::runtime_error(std::string("nfl(hip): ") + what + ": the digit width is out of range");
  P *tmp = P::make_temp();  // (in may be an element of out)
  std::memcpy(static_cast<void *>(tmp->data()), in.cdata(), sizeof(P));
  int rc;
  if (flags >= 0) {
    rc = nflhip_decompose(P::ctx(), out->data(), NFLHIP_FMT_WORDS, tmp->cdata(), 1, w, flags);
  } else {  // no staged entry: a device buffer of the call, on the null stream
    void *d = nullptr;
    rc = nflhip_malloc(P::ctx(), &d, (terms + 1) * sizeof(P));
    if (rc == 0) {
      void *o = static_cast<char *>(d) + sizeof(P);
      rc = nflhip_memcpy_h2d(P::ctx(), d, tmp->cdata(), sizeof(P), nullptr);
      if (rc == 0) rc = nflhip_gadget_mul_dev(P::ctx(), o, d, 1, w, nullptr);
      if (rc == 0) rc = nflhip_memcpy_d2h(P::ctx(), out->data(), o, terms * sizeof(P), nullptr);
      const int rs = nflhip_stream_sync(P::ctx(), nullptr);
      if (rc == 0) rc = rs;
      nflhip_free(P::ctx(), d);
    }
  }
  P::drop_temp(tmp);
  check(P::ctx(), rc, what);
}
}  // namespace detail
template <class T, size_t D, size_t M> void decompose(poly<T, D, M> *out, poly<T, D, M> const &in, int w, bool signed_digits = false) {
  detail::decompose_host(out, in, w, NFLHIP_FORM_COEFF | (signed_digits ? NFLHIP_DECOMP_SIGNED : 0));
}
template <class T, size_t D, size_t M> void decompose_ntt(poly<T, D, M> *out, poly<T, D, M> const &in, int w, bool signed_digits = false) {
  detail::decompose_host(out, in, w, NFLHIP_FORM_NTT | (signed_digits ? NFLHIP_DECOMP_SIGNED : 0));
}
template <class T, size_t D, size_t M> void gadget_mul(poly<T, D, M> *out, poly<T, D, M> const &in, int w) { detail::decompose_host(out, in, w, -1); }
template <class T, size_t D, size_t M> void decompose(poly_p<T, D, M> *out, poly_p<T, D, M> const &in, int w, bool signed_digits = false) {
  poly_p<T, D, M>::decompose_into(out, in, w, NFLHIP_FORM_COEFF | (signed_digits ? NFLHIP_DECOMP_SIGNED : 0));
}
template <class T, size_t D, size_t M> void decompose_ntt(poly_p<T, D, M> *out, poly_p<T, D, M> const &in, int w, bool signed_digits = false) {
  poly_p<T, D, M>::decompose_into(out, in, w, NFLHIP_FORM_NTT | (signed_digits ? NFLHIP_DECOMP_SIGNED : 0));
}
template <class T, size_t D, size_t M> void gadget_mul(poly_p<T, D, M> *out, poly_p<T, D, M> const &in, int w) { poly_p<T, D, M>::decompose_into(out, in, w, -1); }

/* high level wrappers (poly.hpp:314-332) */
template <class T, size_t D, size_t M> void sub(poly<T, D, M> &out, poly<T, D, M> const &a, poly<T, D, M> const &b) { out = a - b; }
template <class T, size_t D, size_t M> void add(poly<T, D, M> &out, poly<T, D, M> const &a, poly<T, D, M> const &b) { out = a + b; }
template <class T, size_t D, size_t M> void mul(poly<T, D, M> &out, poly<T, D, M> const &a, poly<T, D, M> const &b) { out = a * b; }

template <class T, size_t Degree, size_t AggregatedModulusBitSize>
using poly_from_modulus = poly<T, Degree, AggregatedModulusBitSize / params<T>::kModulusBitsize>;

// same text format as the reference's stream operator (core.hpp:398-421)
template <class T, size_t D, size_t M> std::ostream &operator<<(std::ostream &os, poly<T, D, M> const &p) {
  const char *term = sizeof(T) == 8 ? "ULL" : (sizeof(T) == 4 ? "UL" : "U");
  bool first = true;
  os << "{ ";
  for (auto v : p) {
    if (first) { first = false; os << uint64_t(v); }
    else os << term << ", " << uint64_t(v);
  }
  return os << term << " }";
}

}  // namespace nfl
#endif  // NFL_HIP_POLY_P_HPP
