// nfl_hip/batch.hpp -- part of the drop-in header; include <nfl_hip/nfl.hpp> (or the reference's names under include/nfl*).
// batch entry points, nfl::device_batch, nfl::sharded_batch.
#ifndef NFL_HIP_BATCH_HPP
#define NFL_HIP_BATCH_HPP
#ifndef NFL_HIP_NFL_HPP
#error "include <nfl_hip/nfl.hpp>: the parts depend on each other in its order"
#endif
namespace nfl {
// ---------------------------------------------------------------- batch entry points
// A contiguous array of polys is the dense [batch][NbModuli][Degree] tensor the
// device wants (sizeof(poly) == N*sizeof(T)): one H2D, one kernel pass, one D2H.
namespace batch {
template <class P> void ntt_pow_phi(P *first, size_t count) {
  static_assert(sizeof(P) == P::degree * P::nmoduli * sizeof(typename P::value_type), "dense poly array");
  detail::check(P::ctx(), nflhip_ntt_fwd(P::ctx(), first->data(), count), "batch::ntt_pow_phi");
}
template <class P> void invntt_pow_invphi(P *first, size_t count) {
  detail::check(P::ctx(), nflhip_ntt_inv(P::ctx(), first->data(), count), "batch::invntt_pow_invphi");
}
// c[k] = INTT(NTT(a[k]) (.) NTT(b[k])): the fused metric path
template <class P> void polymul(P *c, P const *a, P const *b, size_t count) {
  detail::check(P::ctx(), nflhip_polymul(P::ctx(), c->data(), a->cdata(), b->cdata(), count), "batch::polymul");
}
template <class P> void pointwise(int op, P *out, P const *a, P const *b, P const *bprime, size_t count) {
  detail::check(P::ctx(), nflhip_pointwise(P::ctx(), op, out->data(), a->cdata(), b ? b->cdata() : nullptr,
                                           bprime ? bprime->cdata() : nullptr, count), "batch::pointwise");
}
}  // namespace batch

// ---------------------------------------------------------------- device-resident batches
// The reference's poly stores its words inline on the host (poly.hpp:87-88), so every per-poly call
// above crosses PCIe twice.  device_batch<P> keeps a dense [count][NbModuli][Degree] tensor resident
// in HBM (the role poly_p's shared payload plays on the host, poly_p.hpp:11-204) and runs the same
// operations through the *_dev entry points on one stream: upload once, compute, download once.
// device_batch(count, device) puts it on a GPU of its choice (default: the per-polynomial surface's device).
template <class P> class device_batch {
 public:
  typedef typename P::value_type value_type;
  typedef detail::context<value_type, P::degree, P::nmoduli> context_type;
  explicit device_batch(size_t count) : device_batch(count, detail::default_device().load()) {}
  device_batch(size_t count, int device) : n_(count), d_(nullptr), c_(&context_type::on(device)) {
    static_assert(sizeof(P) == P::degree * P::nmoduli * sizeof(value_type), "dense poly array");
    detail::check(ctx(), nflhip_malloc(ctx(), &d_, bytes()), "device_batch");
  }
  device_batch(const P *host, size_t count) : device_batch(count) { upload(host); }
  ~device_batch() {
    if (small_) nflhip_free(ctx(), small_);
    if (d_) nflhip_free(ctx(), d_);
  }
  device_batch(const device_batch &) = delete;
  device_batch &operator=(const device_batch &) = delete;
  device_batch(device_batch &&o) noexcept : n_(o.n_), d_(o.d_), c_(o.c_), small_(o.small_), small_cap_(o.small_cap_) {
    o.d_ = nullptr;
    o.small_ = nullptr;
    o.small_cap_ = 0;
  }

  size_t size() const { return n_; }
  size_t bytes() const { return n_ * sizeof(P); }
  void *data() { return d_; }
  const void *data() const { return d_; }
  int device() const { return c_->device; }
  nflhip_ctx *ctx() const { return c_->ctx; }     // the context of this batch's device ...
  void *queue() const { return c_->stream; }      // ... and the stream its operations are enqueued on

  void upload(const P *host) {
    detail::check(ctx(), nflhip_memcpy_h2d(ctx(), d_, host->cdata(), bytes(), queue()), "upload");
    sync();
  }
  void download(P *host) const {
    detail::check(ctx(), nflhip_memcpy_d2h(ctx(), host->data(), d_, bytes(), queue()), "download");
    sync();
  }
  void sync() const { detail::check(ctx(), nflhip_stream_sync(ctx(), queue()), "sync"); }

  // same names and meaning as the poly members (poly.hpp:167-168), over the whole batch
  void strict(const char *what) const {   // CHECK_STRICTMOD's assertion over the whole resident batch
    if (detail::strictmod) detail::strict_dev(ctx(), d_, n_, queue(), what);
  }
  void ntt_pow_phi() {
    strict("ntt_pow_phi");
    detail::check(ctx(), nflhip_ntt_fwd_dev(ctx(), d_, n_, queue()), "ntt_pow_phi");
  }
  void invntt_pow_invphi() {
    strict("invntt_pow_invphi");
    detail::check(ctx(), nflhip_ntt_inv_dev(ctx(), d_, n_, queue()), "invntt_pow_invphi");
  }
  // *this = op(a, b[, b'])  (NFLHIP_OP_*); aliasing allowed
  void assign(int op, const device_batch &a, const device_batch &b) {
    same_size(a); same_size(b);
    a.strict("pointwise"); b.strict("pointwise");
    detail::check(ctx(), nflhip_pointwise_dev(ctx(), op, d_, a.d_, b.d_, nullptr, n_, queue()), "pointwise");
  }
  void assign_mul_shoup(const device_batch &a, const device_batch &b, const device_batch &bprime) {
    same_size(a); same_size(b); same_size(bprime);
    a.strict("mulmod_shoup"); b.strict("mulmod_shoup");
    detail::check(ctx(), nflhip_pointwise_dev(ctx(), NFLHIP_OP_MUL_SHOUP, d_, a.d_, b.d_, bprime.d_, n_, queue()),
                  "mulmod_shoup");
  }
  void assign_compute_shoup(const device_batch &b) {
    same_size(b);
    detail::check(ctx(), nflhip_pointwise_dev(ctx(), NFLHIP_OP_COMPUTE_SHOUP, d_, b.d_, nullptr, nullptr, n_, queue()),
                  "compute_shoup");
  }
  // *this = INTT(NTT(a) (.) NTT(b)), the fused metric path
  void assign_polymul(const device_batch &a, const device_batch &b) {
    same_size(a); same_size(b);
    detail::check(ctx(), nflhip_polymul_dev(ctx(), d_, a.d_, b.d_, n_, queue()), "polymul");
  }
  // the same with b already in NTT form (keys of the LWE demo stay transformed, tests/nfllib_demo_main_op.cpp:26-46)
  void assign_polymul_ntt(const device_batch &a, const device_batch &b_ntt) {
    same_size(a); same_size(b_ntt);
    detail::check(ctx(), nflhip_polymul_ntt_dev(ctx(), d_, a.d_, b_ntt.d_, n_, queue()), "polymul_ntt");
  }
  // Galois automorphisms (include/nflhip.h): *this = sigma_k(src), coefficient or NTT form; src must be another batch
  void assign_automorphism(const device_batch &src, uint64_t k, bool ntt_form = false) {
    same_size(src);
    detail::check(ctx(), nflhip_automorphism_dev(ctx(), d_, src.d_, n_, k, ntt_form ? NFLHIP_FORM_NTT : NFLHIP_FORM_COEFF, queue()),
                  "automorphism");
  }
  // *outs[m] = sigma_{ks[m]}(src) for m < count <= NFLHIP_AUTOMORPHISM_MAX_OUTPUTS, one launch that reads src once
  static void assign_automorphisms(device_batch *const *outs, const uint64_t *ks, size_t count, const device_batch &src,
                                   bool ntt_form = false) {
    if (count > NFLHIP_AUTOMORPHISM_MAX_OUTPUTS) throw std::runtime_error("nfl(hip): too many automorphism outputs");
    void *d[NFLHIP_AUTOMORPHISM_MAX_OUTPUTS];
    for (size_t m = 0; m < count; ++m) {
      src.same_size(*outs[m]);
      if (outs[m]->ctx() != src.ctx()) throw std::runtime_error("nfl(hip): automorphism outputs on another device");
      d[m] = outs[m]->d_;
    }
    detail::check(src.ctx(), nflhip_automorphism_multi_dev(src.ctx(), d, ks, count, src.d_, src.n_,
                                                           ntt_form ? NFLHIP_FORM_NTT : NFLHIP_FORM_COEFF, src.queue()),
                  "automorphisms");
  }
  // RNS rescale (include/nflhip.h): *this = round(src / q), q the last modulus of src's ring, which has one modulus more than
  // this batch's.  The two ring types own different streams: this batch's earlier work is awaited, the launch goes on src's
  // stream, and the call returns once it has finished there, so later work on either batch sees the result.
  template <class Q> void assign_rescale(const device_batch<Q> &src, bool ntt_form = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && Q::nmoduli == P::nmoduli + 1,
                  "assign_rescale: the source ring has the same limbs and degree and exactly one modulus more");
    if (src.size() != n_) throw std::runtime_error("nfl(hip): batch sizes differ");
    if (src.device() != device()) throw std::runtime_error("nfl(hip): rescale operands on different devices");
    sync();
    src.strict("rescale");
    detail::check(src.ctx(), nflhip_rescale_dev(src.ctx(), d_, src.data(), n_, ntt_form ? NFLHIP_FORM_NTT : NFLHIP_FORM_COEFF, src.queue()),
                  "rescale");
    src.sync();
  }
  // RNS base conversion (include/nflhip.h), coefficient form: rows [d0, d0 + kd) of this batch become the conversion of rows
  // [s0, s0 + ks) of src -- this batch itself (in place, the mod-up) or another batch of the same ring, in which case the other
  // rows of this batch stay as they are.  assign_mod_down: *this = round(src / P) (floor: floor(src / P) - u), P the product of the
  // last K moduli of src's ring, K = the difference of the two rings' modulus counts; streams ordered as in assign_rescale.
  // ntt_form: both batches hold NTT-form values (the NTT-form entries: the same maps between the transforms).
  void assign_base_convert(const device_batch &src, size_t s0, size_t ks, size_t d0, size_t kd, bool centered = false, bool ntt_form = false) {
    same_size(src);
    if (&src != this) same_device(src);
    src.strict("base_convert");
    const int flags = centered ? NFLHIP_BASECONV_CENTERED : 0;
    if (ntt_form) detail::check(ctx(), nflhip_baseconv_ntt_dev(ctx(), d_, src.d_, n_, s0, ks, d0, kd, flags, queue()), "base_convert_ntt");
    else detail::check(ctx(), nflhip_baseconv_dev(ctx(), d_, src.d_, n_, s0, ks, d0, kd, flags, queue()), "base_convert");
  }
  template <class Q> void assign_mod_down(const device_batch<Q> &src, bool floor = false, bool ntt_form = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && Q::nmoduli > P::nmoduli,
                  "assign_mod_down: the source ring has the same limbs and degree and at least one modulus more");
    if (src.size() != n_) throw std::runtime_error("nfl(hip): batch sizes differ");
    if (src.device() != device()) throw std::runtime_error("nfl(hip): mod_down operands on different devices");
    sync();
    src.strict("mod_down");
    const int flags = floor ? NFLHIP_MODDOWN_FLOOR : 0;
    if (ntt_form) detail::check(src.ctx(), nflhip_moddown_ntt_dev(src.ctx(), d_, src.data(), n_, Q::nmoduli - P::nmoduli, flags, src.queue()), "mod_down_ntt");
    else detail::check(src.ctx(), nflhip_moddown_dev(src.ctx(), d_, src.data(), n_, Q::nmoduli - P::nmoduli, flags, src.queue()), "mod_down");
    src.sync();
  }
  // Hybrid key switch in NTT form (include/nflhip.h "hybrid key switching"): out0, out1 and src are batches of this ring (L
  // moduli) of one size, key a batch of the ring with M > L moduli holding the 2 dnum key polynomials in [term][component] order,
  // shared by the whole batch; K = M - L special moduli, dnum = ceil(L / alpha).  Streams as in assign_mod_down: this ring's work
  // is awaited, the launches go on the key ring's stream, and the call returns once they have finished there.
  template <class Q>
  static void assign_key_switch(device_batch &out0, device_batch &out1, const device_batch &src, const device_batch<Q> &key, size_t alpha,
                                bool centered = false, bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && Q::nmoduli > P::nmoduli,
                  "assign_key_switch: the key's ring has the same limbs and degree and at least one modulus more");
    if (alpha == 0 || alpha > P::nmoduli) throw std::runtime_error("nfl(hip): key_switch: alpha is out of range (1 to the input's moduli)");
    if (out0.size() != src.size() || out1.size() != src.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
    if (key.size() != 2 * ((P::nmoduli + alpha - 1) / alpha)) throw std::runtime_error("nfl(hip): the key batch holds 2 * dnum polynomials");
    if (out0.device() != key.device() || out1.device() != key.device() || src.device() != key.device())
      throw std::runtime_error("nfl(hip): key_switch operands on different devices");
    src.sync();
    src.strict("key_switch");
    key.strict("key_switch");
    const int flags = (centered ? NFLHIP_KEYSWITCH_CENTERED : 0) | (floor ? NFLHIP_KEYSWITCH_FLOOR : 0);
    detail::check(key.ctx(), nflhip_keyswitch_ntt_dev(key.ctx(), out0.d_, out1.d_, src.d_, key.data(), src.n_, Q::nmoduli - P::nmoduli, alpha, flags,
                                                      key.queue()), "key_switch_ntt");
    key.sync();
  }
  // Hoisted rotations (include/nflhip.h "hoisted rotations"): c0 (may be NULL), c1 and every out0s[m], out1s[m] are batches of this
  // ring (L moduli) of one size; key_batches[m] is a batch of the ring with M > L moduli holding the 2 dnum polynomials of the key of
  // rotation m in [term][component] order, shared by the whole batch; K = M - L special moduli, dnum = ceil(L / alpha); m < count
  // <= 16.  Streams as in assign_key_switch: this ring's work is awaited, the launches go on the key ring's stream (that of
  // key_batches[0]), and the call returns once they have finished there.
  template <class Q>
  static void assign_rotations(device_batch *const *out0s, device_batch *const *out1s, const device_batch *c0, const device_batch &c1,
                               const device_batch<Q> *const *key_batches, const uint64_t *ks, size_t count, size_t alpha, bool centered = false,
                               bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && Q::nmoduli > P::nmoduli,
                  "assign_rotations: the keys' ring has the same limbs and degree and at least one modulus more");
    if (alpha == 0 || alpha > P::nmoduli) throw std::runtime_error("nfl(hip): rotations: alpha is out of range (1 to the ciphertext's moduli)");
    if (count == 0 || count > NFLHIP_ROTATE_MAX_OUTPUTS) throw std::runtime_error("nfl(hip): rotations: 1 to 16 rotations");
    const device_batch<Q> &key0 = *key_batches[0];
    void *o0[NFLHIP_ROTATE_MAX_OUTPUTS], *o1[NFLHIP_ROTATE_MAX_OUTPUTS];
    const void *kp[NFLHIP_ROTATE_MAX_OUTPUTS];
    if (c0 && c0->size() != c1.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
    if ((c0 && c0->device() != key0.device()) || c1.device() != key0.device()) throw std::runtime_error("nfl(hip): rotation operands on different devices");
    for (size_t m = 0; m < count; ++m) {
      if (out0s[m]->size() != c1.size() || out1s[m]->size() != c1.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
      if (key_batches[m]->size() != 2 * ((P::nmoduli + alpha - 1) / alpha)) throw std::runtime_error("nfl(hip): a key batch holds 2 * dnum polynomials");
      if (out0s[m]->device() != key0.device() || out1s[m]->device() != key0.device() || key_batches[m]->device() != key0.device())
        throw std::runtime_error("nfl(hip): rotation operands on different devices");
      o0[m] = out0s[m]->d_;
      o1[m] = out1s[m]->d_;
      kp[m] = key_batches[m]->data();
    }
    c1.sync();
    c1.strict("rotations");
    if (c0) c0->strict("rotations");
    for (size_t m = 0; m < count; ++m) key_batches[m]->strict("rotations");
    const int flags = (centered ? NFLHIP_ROTATE_CENTERED : 0) | (floor ? NFLHIP_ROTATE_FLOOR : 0);
    detail::check(key0.ctx(), nflhip_rotate_hoisted_ntt_dev(key0.ctx(), o0, o1, c0 ? c0->d_ : nullptr, c1.d_, kp, ks, count, c1.n_,
                                                            Q::nmoduli - P::nmoduli, alpha, flags, key0.queue()), "rotate_hoisted_ntt");
    key0.sync();
  }
  // Slot linear transforms (include/nflhip.h "slot linear transforms"): c0 (may be NULL), c1, out0 and out1 are batches of this ring (L
  // moduli) of one size; key_batches[m] as for assign_rotations, or NULL for the unrotated diagonal (ks[m] = 1); weight_batches[m] is a
  // batch of the keys' ring holding the one polynomial of diagonal m, shared by the whole batch; m < count <= 16.  Streams as in
  // assign_rotations: the launches go on the key ring's stream (that of weight_batches[0]), and the call returns once they have
  // finished there.
  template <class Q>
  static void assign_linear_transform(device_batch &out0, device_batch &out1, const device_batch *c0, const device_batch &c1,
                                      const device_batch<Q> *const *key_batches, const device_batch<Q> *const *weight_batches, const uint64_t *ks,
                                      size_t count, size_t alpha, bool centered = false, bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && Q::nmoduli > P::nmoduli,
                  "assign_linear_transform: the keys' ring has the same limbs and degree and at least one modulus more");
    if (alpha == 0 || alpha > P::nmoduli) throw std::runtime_error("nfl(hip): linear transform: alpha is out of range (1 to the ciphertext's moduli)");
    if (count == 0 || count > NFLHIP_LINTRANS_MAX_TERMS) throw std::runtime_error("nfl(hip): linear transform: 1 to 16 terms");
    const device_batch<Q> &w0 = *weight_batches[0];
    const void *kp[NFLHIP_LINTRANS_MAX_TERMS], *wp[NFLHIP_LINTRANS_MAX_TERMS];
    if ((c0 && c0->size() != c1.size()) || out0.size() != c1.size() || out1.size() != c1.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
    if ((c0 && c0->device() != w0.device()) || c1.device() != w0.device() || out0.device() != w0.device() || out1.device() != w0.device())
      throw std::runtime_error("nfl(hip): linear transform operands on different devices");
    for (size_t m = 0; m < count; ++m) {
      if (key_batches[m] && key_batches[m]->size() != 2 * ((P::nmoduli + alpha - 1) / alpha)) throw std::runtime_error("nfl(hip): a key batch holds 2 * dnum polynomials");
      if (weight_batches[m]->size() != 1) throw std::runtime_error("nfl(hip): a weight batch holds one polynomial");
      if ((key_batches[m] && key_batches[m]->device() != w0.device()) || weight_batches[m]->device() != w0.device())
        throw std::runtime_error("nfl(hip): linear transform operands on different devices");
      kp[m] = key_batches[m] ? key_batches[m]->data() : nullptr;
      wp[m] = weight_batches[m]->data();
    }
    c1.sync();
    c1.strict("linear transform");
    if (c0) c0->strict("linear transform");
    for (size_t m = 0; m < count; ++m) {
      if (key_batches[m]) key_batches[m]->strict("linear transform");
      weight_batches[m]->strict("linear transform");
    }
    const int flags = (centered ? NFLHIP_LINTRANS_CENTERED : 0) | (floor ? NFLHIP_LINTRANS_FLOOR : 0);
    detail::check(w0.ctx(), nflhip_lintrans_ntt_dev(w0.ctx(), out0.d_, out1.d_, c0 ? c0->d_ : nullptr, c1.d_, kp, wp, ks, count, c1.n_,
                                                    Q::nmoduli - P::nmoduli, alpha, flags, w0.queue()), "linear_transform_ntt");
    w0.sync();
  }
  // Ciphertext multiplication with relinearisation (include/nflhip.h "ciphertext multiplication"): a0, a1, b0, b1 are batches of this
  // ring (L moduli) of one size -- b0 == b1 == NULL: the square --, key a batch of the ring with M > L moduli holding the 2 dnum
  // polynomials of the key from s^2 to s in [term][component] order, shared by the whole batch.  out0, out1 are batches of this ring,
  // or of the ring with L - 1 moduli: then the result is rescaled by the last kept modulus in the same rounding.  An output may be
  // one of the inputs.  Streams as in assign_key_switch.
  template <class O, class Q>
  static void assign_mul_relin(device_batch<O> &out0, device_batch<O> &out1, const device_batch &a0, const device_batch &a1, const device_batch *b0,
                               const device_batch *b1, const device_batch<Q> &key, size_t alpha, bool centered = false, bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && Q::nmoduli > P::nmoduli,
                  "assign_mul_relin: the key's ring has the same limbs and degree and at least one modulus more");
    static_assert(std::is_same<typename O::value_type, value_type>::value && O::degree == P::degree &&
                      (O::nmoduli == P::nmoduli || O::nmoduli + 1 == P::nmoduli),
                  "assign_mul_relin: the outputs live in the inputs' ring, or in the ring with one modulus less (the rescale)");
    if (alpha == 0 || alpha > P::nmoduli) throw std::runtime_error("nfl(hip): mul_relin: alpha is out of range (1 to the inputs' moduli)");
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): mul_relin: b0 and b1 are both given, or both NULL for the square");
    if (out0.size() != a0.size() || out1.size() != a0.size() || a1.size() != a0.size() || (b0 && (b0->size() != a0.size() || b1->size() != a0.size())))
      throw std::runtime_error("nfl(hip): batch sizes differ");
    if (key.size() != 2 * ((P::nmoduli + alpha - 1) / alpha)) throw std::runtime_error("nfl(hip): the key batch holds 2 * dnum polynomials");
    if (out0.device() != key.device() || out1.device() != key.device() || a0.device() != key.device() || a1.device() != key.device() ||
        (b0 && (b0->device() != key.device() || b1->device() != key.device())))
      throw std::runtime_error("nfl(hip): mul_relin operands on different devices");
    a0.sync();
    out0.sync();
    a0.strict("mul_relin"), a1.strict("mul_relin"), key.strict("mul_relin");
    if (b0) b0->strict("mul_relin"), b1->strict("mul_relin");
    const int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0) |
                      (O::nmoduli != P::nmoduli ? NFLHIP_MULRELIN_RESCALE : 0);
    detail::check(key.ctx(), nflhip_mulrelin_ntt_dev(key.ctx(), out0.data(), out1.data(), a0.d_, a1.d_, b0 ? b0->d_ : nullptr, b1 ? b1->d_ : nullptr,
                                                     key.data(), a0.n_, Q::nmoduli - P::nmoduli, alpha, flags, key.queue()), "mul_relin_ntt");
    key.sync();
  }
  // The two at a level (include/nflhip.h "leveled key switching"): this ring's moduli count is the level Lv, and `key` is a batch of the
  // ring with M moduli holding the 2 dnum_L polynomials of the ONE top-level key, of which the first 2 ceil(Lv / alpha) are read.  The
  // last K moduli of the key's ring are the special ones: K cannot be deduced from the types any more, so it is explicit, and
  // Lv <= M - K is checked at compile time.  Streams as in assign_key_switch.
  template <size_t K, class Q>
  static void assign_key_switch_level(device_batch &out0, device_batch &out1, const device_batch &src, const device_batch<Q> &key, size_t alpha,
                                      bool centered = false, bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && K >= 1 && K < Q::nmoduli &&
                      P::nmoduli <= Q::nmoduli - K,
                  "assign_key_switch_level: the key's ring has the same limbs and degree, K special moduli and at least Lv others");
    if (alpha == 0 || alpha > Q::nmoduli - K) throw std::runtime_error("nfl(hip): key_switch_level: alpha is out of range (1 to the key's ordinary moduli)");
    if (out0.size() != src.size() || out1.size() != src.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
    if (key.size() != 2 * ((Q::nmoduli - K + alpha - 1) / alpha)) throw std::runtime_error("nfl(hip): the key batch holds the 2 * dnum polynomials of the top level");
    if (out0.device() != key.device() || out1.device() != key.device() || src.device() != key.device())
      throw std::runtime_error("nfl(hip): key_switch_level operands on different devices");
    src.sync();
    src.strict("key_switch_level");
    key.strict("key_switch_level");
    int flags = centered ? NFLHIP_KEYSWITCH_CENTERED : 0;
    if (floor) flags |= NFLHIP_KEYSWITCH_FLOOR;
    detail::check(key.ctx(), nflhip_keyswitch_level_ntt_dev(key.ctx(), out0.d_, out1.d_, src.d_, key.data(), src.n_, K, alpha, P::nmoduli, flags,
                                                            key.queue()), "key_switch_level_ntt");
    key.sync();
  }
  template <size_t K, class O, class Q>
  static void assign_mul_relin_level(device_batch<O> &out0, device_batch<O> &out1, const device_batch &a0, const device_batch &a1,
                                     const device_batch *b0, const device_batch *b1, const device_batch<Q> &key, size_t alpha, bool centered = false,
                                     bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && K >= 1 && K < Q::nmoduli &&
                      P::nmoduli <= Q::nmoduli - K,
                  "assign_mul_relin_level: the key's ring has the same limbs and degree, K special moduli and at least Lv others");
    static_assert(std::is_same<typename O::value_type, value_type>::value && O::degree == P::degree &&
                      (O::nmoduli == P::nmoduli || O::nmoduli + 1 == P::nmoduli),
                  "assign_mul_relin_level: the outputs live in the inputs' ring, or in the ring with one modulus less (the rescale)");
    if (alpha == 0 || alpha > Q::nmoduli - K) throw std::runtime_error("nfl(hip): mul_relin_level: alpha is out of range (1 to the key's ordinary moduli)");
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): mul_relin_level: b0 and b1 are both given, or both NULL for the square");
    if (out0.size() != a0.size() || out1.size() != a0.size() || a1.size() != a0.size() || (b0 && (b0->size() != a0.size() || b1->size() != a0.size())))
      throw std::runtime_error("nfl(hip): batch sizes differ");
    if (key.size() != 2 * ((Q::nmoduli - K + alpha - 1) / alpha)) throw std::runtime_error("nfl(hip): the key batch holds the 2 * dnum polynomials of the top level");
    if (out0.device() != key.device() || out1.device() != key.device() || a0.device() != key.device() || a1.device() != key.device() ||
        (b0 && (b0->device() != key.device() || b1->device() != key.device())))
      throw std::runtime_error("nfl(hip): mul_relin_level operands on different devices");
    a0.sync();
    out0.sync();
    a0.strict("mul_relin_level"), a1.strict("mul_relin_level"), key.strict("mul_relin_level");
    if (b0) b0->strict("mul_relin_level"), b1->strict("mul_relin_level");
    int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0);
    if (O::nmoduli != P::nmoduli) flags |= NFLHIP_MULRELIN_RESCALE;
    const void *const x0 = b0 ? b0->d_ : nullptr, *const x1 = b1 ? b1->d_ : nullptr;
    detail::check(key.ctx(), nflhip_mulrelin_level_ntt_dev(key.ctx(), out0.data(), out1.data(), a0.d_, a1.d_, x0, x1, key.data(), a0.n_, K, alpha,
                                                           P::nmoduli, flags, key.queue()), "mul_relin_level_ntt");
    key.sync();
  }
  // Sums of ciphertext products at a level (include/nflhip.h "sums of ciphertext products"): a0, a1 hold groups * terms polynomials,
  // [group][term]; b0, b1 alike, or `terms` polynomials shared by every group with b_shared (both NULL: the sums of squares); the
  // outputs hold `groups` polynomials and their ring decides the rescale, as in assign_mul_relin.  The key, K and the level as in
  // assign_mul_relin_level; Lv = M - K is the top level.  Streams as in assign_key_switch.
  template <size_t K, class O, class Q>
  static void assign_mul_relin_dot_level(device_batch<O> &out0, device_batch<O> &out1, const device_batch &a0, const device_batch &a1,
                                         const device_batch *b0, const device_batch *b1, size_t terms, const device_batch<Q> &key, size_t alpha,
                                         bool b_shared = false, bool centered = false, bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && K >= 1 && K < Q::nmoduli &&
                      P::nmoduli <= Q::nmoduli - K,
                  "assign_mul_relin_dot_level: the key's ring has the same limbs and degree, K special moduli and at least Lv others");
    static_assert(std::is_same<typename O::value_type, value_type>::value && O::degree == P::degree &&
                      (O::nmoduli == P::nmoduli || O::nmoduli + 1 == P::nmoduli),
                  "assign_mul_relin_dot_level: the outputs live in the inputs' ring, or in the ring with one modulus less (the rescale)");
    if (alpha == 0 || alpha > Q::nmoduli - K) throw std::runtime_error("nfl(hip): mul_relin_dot_level: alpha is out of range (1 to the key's ordinary moduli)");
    if (!b0 != !b1) throw std::runtime_error("nfl(hip): mul_relin_dot_level: b0 and b1 are both given, or both NULL for the squares");
    if (terms == 0 || a0.size() % terms) throw std::runtime_error("nfl(hip): mul_relin_dot_level: a0 holds groups * terms polynomials");
    const size_t groups = a0.size() / terms;
    if (out0.size() != groups || out1.size() != groups || a1.size() != a0.size() ||
        (b0 && (b0->size() != (b_shared ? terms : a0.size()) || b1->size() != b0->size())))
      throw std::runtime_error("nfl(hip): batch sizes differ");
    if (key.size() != 2 * ((Q::nmoduli - K + alpha - 1) / alpha)) throw std::runtime_error("nfl(hip): the key batch holds the 2 * dnum polynomials of the top level");
    if (out0.device() != key.device() || out1.device() != key.device() || a0.device() != key.device() || a1.device() != key.device() ||
        (b0 && (b0->device() != key.device() || b1->device() != key.device())))
      throw std::runtime_error("nfl(hip): mul_relin_dot_level operands on different devices");
    a0.sync();
    out0.sync();
    a0.strict("mul_relin_dot_level"), a1.strict("mul_relin_dot_level"), key.strict("mul_relin_dot_level");
    if (b0) b0->strict("mul_relin_dot_level"), b1->strict("mul_relin_dot_level");
    const int rescale = O::nmoduli != P::nmoduli ? NFLHIP_MULRELIN_RESCALE : 0;
    const int flags = (centered ? NFLHIP_MULRELIN_CENTERED : 0) | (floor ? NFLHIP_MULRELIN_FLOOR : 0) | rescale;
    const nflhip_dot_operand x0 = {a0.d_, terms, 1}, x1 = {a1.d_, terms, 1};
    const nflhip_dot_operand y0 = {b0 ? b0->d_ : nullptr, b_shared ? 0 : terms, 1}, y1 = {b1 ? b1->d_ : nullptr, b_shared ? 0 : terms, 1};
    detail::check(key.ctx(), nflhip_mulrelin_dot_ntt_dev(key.ctx(), out0.data(), out1.data(), &x0, &x1, b0 ? &y0 : nullptr, b1 ? &y1 : nullptr, key.data(),
                                                         groups, terms, K, alpha, P::nmoduli, flags, key.queue()), "mul_relin_dot_level_ntt");
    key.sync();
  }
  // Hoisted rotations and slot linear transforms at a level (include/nflhip.h "rotations and linear transforms at a level"): this
  // ring's moduli count is the level Lv; key_batches[m] is a batch of the ring with M moduli holding the 2 dnum_L polynomials of the ONE
  // top-level Galois key of rotation m (NULL: the unrotated diagonal of a linear transform), weight_batches[m] one holding the ONE
  // top-level diagonal.  The last K moduli of the keys' ring are the special ones, K explicit as in nfl::rotate_hoisted_level_ntt<K>;
  // Lv <= M - K is checked at compile time.  Streams as in assign_rotations / assign_linear_transform.
  template <size_t K, class Q>
  static void assign_rotations_level(device_batch *const *out0s, device_batch *const *out1s, const device_batch *c0, const device_batch &c1,
                                     const device_batch<Q> *const *key_batches, const uint64_t *ks, size_t count, size_t alpha, bool centered = false,
                                     bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && K >= 1 && K < Q::nmoduli &&
                      P::nmoduli <= Q::nmoduli - K,
                  "assign_rotations_level: the keys' ring has the same limbs and degree, K special moduli and at least Lv others");
    if (alpha == 0 || alpha > Q::nmoduli - K) throw std::runtime_error("nfl(hip): rotations_level: alpha is out of range (1 to the keys' ordinary moduli)");
    if (count == 0 || count > NFLHIP_ROTATE_MAX_OUTPUTS) throw std::runtime_error("nfl(hip): rotations_level: 1 to 16 rotations");
    const device_batch<Q> &key0 = *key_batches[0];
    void *o0[NFLHIP_ROTATE_MAX_OUTPUTS], *o1[NFLHIP_ROTATE_MAX_OUTPUTS];
    const void *kp[NFLHIP_ROTATE_MAX_OUTPUTS];
    if (c0 && c0->size() != c1.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
    if ((c0 && c0->device() != key0.device()) || c1.device() != key0.device()) throw std::runtime_error("nfl(hip): rotation operands on different devices");
    for (size_t m = 0; m < count; ++m) {
      if (out0s[m]->size() != c1.size() || out1s[m]->size() != c1.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
      if (key_batches[m]->size() != 2 * ((Q::nmoduli - K + alpha - 1) / alpha))
        throw std::runtime_error("nfl(hip): a key batch holds the 2 * dnum polynomials of the top level");
      if (out0s[m]->device() != key0.device() || out1s[m]->device() != key0.device() || key_batches[m]->device() != key0.device())
        throw std::runtime_error("nfl(hip): rotation operands on different devices");
      o0[m] = out0s[m]->d_;
      o1[m] = out1s[m]->d_;
      kp[m] = key_batches[m]->data();
    }
    c1.sync();
    c1.strict("rotations_level");
    if (c0) c0->strict("rotations_level");
    for (size_t m = 0; m < count; ++m) key_batches[m]->strict("rotations_level");
    const int flags = (centered ? NFLHIP_ROTATE_CENTERED : 0) | (floor ? NFLHIP_ROTATE_FLOOR : 0);
    const void *const p0 = c0 ? c0->d_ : nullptr;
    detail::check(key0.ctx(), nflhip_rotate_hoisted_level_ntt_dev(key0.ctx(), o0, o1, p0, c1.d_, kp, ks, count, c1.n_, K, alpha,
                                                                  P::nmoduli, flags, key0.queue()), "rotate_hoisted_level_ntt");
    key0.sync();
  }
  template <size_t K, class Q>
  static void assign_linear_transform_level(device_batch &out0, device_batch &out1, const device_batch *c0, const device_batch &c1,
                                            const device_batch<Q> *const *key_batches, const device_batch<Q> *const *weight_batches,
                                            const uint64_t *ks, size_t count, size_t alpha, bool centered = false, bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && K >= 1 && K < Q::nmoduli &&
                      P::nmoduli <= Q::nmoduli - K,
                  "assign_linear_transform_level: the keys' ring has the same limbs and degree, K special moduli and at least Lv others");
    if (alpha == 0 || alpha > Q::nmoduli - K) throw std::runtime_error("nfl(hip): linear transform level: alpha is out of range (1 to the keys' ordinary moduli)");
    if (count == 0 || count > NFLHIP_LINTRANS_MAX_TERMS) throw std::runtime_error("nfl(hip): linear transform level: 1 to 16 terms");
    const device_batch<Q> &w0 = *weight_batches[0];
    const void *kp[NFLHIP_LINTRANS_MAX_TERMS], *wp[NFLHIP_LINTRANS_MAX_TERMS];
    if ((c0 && c0->size() != c1.size()) || out0.size() != c1.size() || out1.size() != c1.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
    if ((c0 && c0->device() != w0.device()) || c1.device() != w0.device() || out0.device() != w0.device() || out1.device() != w0.device())
      throw std::runtime_error("nfl(hip): linear transform operands on different devices");
    for (size_t m = 0; m < count; ++m) {
      if (key_batches[m] && key_batches[m]->size() != 2 * ((Q::nmoduli - K + alpha - 1) / alpha))
        throw std::runtime_error("nfl(hip): a key batch holds the 2 * dnum polynomials of the top level");
      if (weight_batches[m]->size() != 1) throw std::runtime_error("nfl(hip): a weight batch holds one polynomial");
      if ((key_batches[m] && key_batches[m]->device() != w0.device()) || weight_batches[m]->device() != w0.device())
        throw std::runtime_error("nfl(hip): linear transform operands on different devices");
      kp[m] = key_batches[m] ? key_batches[m]->data() : nullptr;
      wp[m] = (*weight_batches[m]).data();
    }
    c1.sync();
    c1.strict("linear transform level");
    if (c0) c0->strict("linear transform level");
    for (size_t m = 0; m < count; ++m) {
      if (key_batches[m]) key_batches[m]->strict("linear transform level");
      weight_batches[m]->strict("linear transform level");
    }
    const int flags = (centered ? NFLHIP_LINTRANS_CENTERED : 0) | (floor ? NFLHIP_LINTRANS_FLOOR : 0);
    const void *const p0 = c0 ? c0->d_ : nullptr;
    detail::check(w0.ctx(), nflhip_lintrans_level_ntt_dev(w0.ctx(), out0.d_, out1.d_, p0, c1.d_, kp, wp, ks, count, c1.n_, K, alpha,
                                                          P::nmoduli, flags, w0.queue()), "linear_transform_level_ntt");
    w0.sync();
  }
  // BSGS slot linear transforms (include/nflhip.h "BSGS slot linear transforms"): this batch type is the ciphertext's at its level;
  // bkey_batches[i] / gkey_batches[j] hold the 2 * dnum_L polynomials of a step's top-level Galois key (NULL: the unrotated step),
  // weight_batches[j * n1 + i] the one top-level diagonal (NULL: the zero diagonal).  Streams as in assign_linear_transform_level.
  template <size_t K, class Q>
  static void assign_bsgs_linear_transform(device_batch &out0, device_batch &out1, const device_batch *c0, const device_batch &c1,
                                           const device_batch<Q> *const *bkey_batches, const uint64_t *bks, size_t n1,
                                           const device_batch<Q> *const *gkey_batches, const uint64_t *gks, size_t n2,
                                           const device_batch<Q> *const *weight_batches, size_t alpha, bool centered = false, bool floor = false) {
    static_assert(std::is_same<typename Q::value_type, value_type>::value && Q::degree == P::degree && K >= 1 && K < Q::nmoduli &&
                      P::nmoduli <= Q::nmoduli - K,
                  "assign_bsgs_linear_transform: the keys' ring has the same limbs and degree, K special moduli and at least Lv others");
    if (alpha == 0 || alpha > Q::nmoduli - K) throw std::runtime_error("nfl(hip): bsgs linear transform: alpha is out of range (1 to the keys' ordinary moduli)");
    if (n1 == 0 || n1 > NFLHIP_BSGS_MAX_BABY || n2 == 0 || n2 > NFLHIP_BSGS_MAX_GIANT) throw std::runtime_error("nfl(hip): bsgs linear transform: 1 to 16 baby and giant steps");
    const device_batch<Q> *w0 = nullptr;
    for (size_t q = 0; q < n1 * n2 && !w0; ++q) w0 = weight_batches[q];
    if (!w0) throw std::runtime_error("nfl(hip): bsgs linear transform: no diagonal");
    const void *bp[NFLHIP_BSGS_MAX_BABY], *gp[NFLHIP_BSGS_MAX_GIANT], *wp[NFLHIP_BSGS_MAX_BABY * NFLHIP_BSGS_MAX_GIANT];
    if ((c0 && c0->size() != c1.size()) || out0.size() != c1.size() || out1.size() != c1.size()) throw std::runtime_error("nfl(hip): batch sizes differ");
    if ((c0 && c0->device() != w0->device()) || c1.device() != w0->device() || out0.device() != w0->device() || out1.device() != w0->device())
      throw std::runtime_error("nfl(hip): bsgs linear transform operands on different devices");
    for (size_t m = 0; m < n1 + n2; ++m) {
      const device_batch<Q> *kb = m < n1 ? bkey_batches[m] : gkey_batches[m - n1];
      if (kb && kb->size() != 2 * ((Q::nmoduli - K + alpha - 1) / alpha)) throw std::runtime_error("nfl(hip): a key batch holds the 2 * dnum polynomials of the top level");
      if (kb && kb->device() != w0->device()) throw std::runtime_error("nfl(hip): bsgs linear transform operands on different devices");
      (m < n1 ? bp[m] : gp[m - n1]) = kb ? kb->data() : nullptr;
    }
    for (size_t q = 0; q < n1 * n2; ++q) {
      const device_batch<Q> *wb = weight_batches[q];
      if (wb && wb->size() != 1) throw std::runtime_error("nfl(hip): a weight batch holds one polynomial");
      if (wb && wb->device() != w0->device()) throw std::runtime_error("nfl(hip): bsgs linear transform operands on different devices");
      wp[q] = wb ? wb->data() : nullptr;
    }
    c1.sync();
    c1.strict("bsgs linear transform");
    if (c0) c0->strict("bsgs linear transform");
    for (size_t m = 0; m < n1 + n2; ++m) {
      const device_batch<Q> *kb = m < n1 ? bkey_batches[m] : gkey_batches[m - n1];
      if (kb) kb->strict("bsgs linear transform");
    }
    for (size_t q = 0; q < n1 * n2; ++q)
      if (weight_batches[q]) weight_batches[q]->strict("bsgs linear transform");
    const int flags = (centered ? NFLHIP_BSGS_CENTERED : 0) | (floor ? NFLHIP_BSGS_FLOOR : 0);
    const void *const p0 = c0 ? c0->d_ : nullptr;
    detail::check(w0->ctx(), nflhip_bsgs_ntt_dev(w0->ctx(), out0.d_, out1.d_, p0, c1.d_, bp, bks, n1, gp, gks, n2, wp, c1.n_, K, alpha,
                                                 P::nmoduli, flags, w0->queue()), "bsgs_linear_transform_ntt");
    w0->sync();
  }
  // Sums of products across polynomials (include/nflhip.h): this batch holds `groups` polynomials, a and b groups * terms each,
  // term-minor: (*this)[g] = sum_j a[g * terms + j] * b[g * terms + j].  assign_matvec: v holds the `terms` polynomials every
  // group shares, (*this)[g] = sum_j m[g * terms + j] * v[j].  The operands must be other batches.
  void assign_dot(const device_batch &a, const device_batch &b, size_t terms) {
    if (terms == 0 || a.n_ != n_ * terms || b.n_ != n_ * terms) throw std::runtime_error("nfl(hip): dot operands hold groups * terms polynomials");
    same_device(a), same_device(b);
    a.strict("dot"); b.strict("dot");
    const nflhip_dot_operand x = {a.d_, terms, 1}, y = {b.d_, terms, 1};
    detail::check(ctx(), nflhip_dot_dev(ctx(), d_, &x, &y, nullptr, n_, terms, 0, queue()), "dot");
  }
  void assign_matvec(const device_batch &m, const device_batch &v) {
    if (v.n_ == 0 || m.n_ != n_ * v.n_) throw std::runtime_error("nfl(hip): the matrix holds groups * terms polynomials, the vector terms");
    same_device(m), same_device(v);
    m.strict("matvec"); v.strict("matvec");
    const nflhip_dot_operand x = {m.d_, v.n_, 1}, y = {v.d_, 0, 1};
    detail::check(ctx(), nflhip_dot_dev(ctx(), d_, &x, &y, nullptr, n_, v.n_, 0, queue()), "matvec");
  }
  // Gadget decomposition (include/nflhip.h): this batch holds src.size() * terms polynomials, terms = nmoduli * ceil(modulus
  // bits / w): (*this)[b * terms + m * l + t] = digit t of row m of the coefficient-form src[b], spread over every row.  flags =
  // NFLHIP_FORM_COEFF or NFLHIP_FORM_NTT, | NFLHIP_DECOMP_SIGNED, | a plan flag.  assign_gadget_mul: the key-generation
  // companion, src[b] * 2^(w t) in row m of the same term, zero elsewhere.  src must be another batch.
  void assign_decompose(const device_batch &src, int w, int flags = NFLHIP_FORM_COEFF) {
    decompose_sizes(src, w);
    src.strict("decompose");
    detail::check(ctx(), nflhip_decompose_dev(ctx(), d_, NFLHIP_FMT_WORDS, src.d_, src.n_, w, flags, queue()), "decompose");
  }
  void assign_gadget_mul(const device_batch &src, int w) {
    decompose_sizes(src, w);
    src.strict("gadget_mul");
    detail::check(ctx(), nflhip_gadget_mul_dev(ctx(), d_, src.d_, src.n_, w, queue()), "gadget_mul");
  }
  // CRT lift / project of the whole resident batch (gmp.hpp:183-219): out[(b*degree + i)*L .. +L) = little-endian limbs
  // of X_{b,i} in [0, Q), L = P::crt_limbs(); limbs2poly takes L_in limbs per coefficient
  void poly2limbs(std::vector<uint64_t> &out) const {
    const size_t words = n_ * P::degree * P::crt_limbs();
    out.assign(words, 0);
    void *dl = nullptr;
    detail::check(ctx(), nflhip_malloc(ctx(), &dl, words * sizeof(uint64_t)), "device allocation");
    int rc = nflhip_crt_lift_dev(ctx(), static_cast<uint64_t *>(dl), d_, n_, queue());
    if (rc == 0) rc = nflhip_memcpy_d2h(ctx(), out.data(), dl, words * sizeof(uint64_t), queue());
    if (rc == 0) rc = nflhip_stream_sync(ctx(), queue());
    nflhip_free(ctx(), dl);
    detail::check(ctx(), rc, "poly2mpz");
  }
  void limbs2poly(const uint64_t *limbs, size_t L_in) {
    const size_t words = n_ * P::degree * L_in;
    void *dl = nullptr;
    detail::check(ctx(), nflhip_malloc(ctx(), &dl, words * sizeof(uint64_t)), "device allocation");
    int rc = nflhip_memcpy_h2d(ctx(), dl, limbs, words * sizeof(uint64_t), queue());
    if (rc == 0) rc = nflhip_crt_project_dev(ctx(), d_, static_cast<const uint64_t *>(dl), L_in, n_, queue());
    if (rc == 0) rc = nflhip_stream_sync(ctx(), queue());
    nflhip_free(ctx(), dl);
    detail::check(ctx(), rc, "mpz2poly");
  }
  // fused postfix expression over up to NFLHIP_EXPR_MAX_OPERANDS resident batches
  void assign_program(const unsigned char *program, size_t len, const device_batch *const *operands, size_t count) {
    const void *ptr[NFLHIP_EXPR_MAX_OPERANDS];
    if (count > NFLHIP_EXPR_MAX_OPERANDS) throw std::runtime_error("nfl(hip): too many operands");
    for (size_t i = 0; i < count; ++i) { same_size(*operands[i]); ptr[i] = operands[i]->d_; }
    if (detail::strictmod) {
      const unsigned skip = detail::strict_exempt(program, len);
      for (size_t i = 0; i < count; ++i)
        if (!(skip >> i & 1)) operands[i]->strict("eval");
    }
    detail::check(ctx(), nflhip_eval_dev(ctx(), d_, ptr, count, program, len, n_, queue()), "eval");
  }
  // the random constructors over the whole resident batch (same tags as poly's; one keystream per call).
  // `first_poly` / `stream_id` are for shards of one logical batch (sharded_batch): polynomial k of this batch is
  // polynomial first_poly + k of the keystream, so that the shards of a batch equal the batch drawn on one device.
  void set(uniform const &u, size_t first_poly = 0) {
    if (u.seeded) detail::check(ctx(), nflhip_fill_uniform_dev(ctx(), d_, first_poly, n_, u.seed, 0, queue()), "set(uniform)");
    else sample(detail::uniform_rule(), 0, 1, "set(uniform)", first_poly, detail::sampler::get().next++);
  }
  void set(non_uniform const &m) { sample(NFLHIP_DIST_BOUNDED, m.upper_bound, m.amplifier, "set(non_uniform)", 0, detail::sampler::get().next++); }
  void set(ZO_dist const &m) { sample(NFLHIP_DIST_ZO | detail::dist_flags, m.rho, 1, "set(ZO_dist)", 0, detail::sampler::get().next++); }
  void set(hwt_dist const &m) { sample(NFLHIP_DIST_HWT | detail::dist_flags, m.hwt, 1, "set(hwt_dist)", 0, detail::sampler::get().next++); }
  template <class in_class, unsigned _lu_depth> void set(gaussian<in_class, value_type, _lu_depth> const &m) {
    set_at(m, 0, detail::sampler::get().next++);
  }
  void set_at(uniform const &, size_t first_poly, uint64_t stream_id) { sample(detail::uniform_rule(), 0, 1, "set(uniform)", first_poly, stream_id); }
  void set_at(non_uniform const &m, size_t first_poly, uint64_t stream_id) { sample(NFLHIP_DIST_BOUNDED, m.upper_bound, m.amplifier, "set(non_uniform)", first_poly, stream_id); }
  void set_at(ZO_dist const &m, size_t first_poly, uint64_t stream_id) { sample(NFLHIP_DIST_ZO | detail::dist_flags, m.rho, 1, "set(ZO_dist)", first_poly, stream_id); }
  void set_at(hwt_dist const &m, size_t first_poly, uint64_t stream_id) { sample(NFLHIP_DIST_HWT | detail::dist_flags, m.hwt, 1, "set(hwt_dist)", first_poly, stream_id); }
  template <class in_class, unsigned _lu_depth>
  void set_at(gaussian<in_class, value_type, _lu_depth> const &m, size_t first_poly, uint64_t stream_id) {
    detail::sampler &s = detail::sampler::get();
    detail::check(ctx(), nflhip_sample_gauss_dev(ctx(), d_, first_poly, n_, m.fg_prng->table(ctx()), m.amplifier, s.key,
                                                 stream_id, queue()), "set(gaussian)");
  }
  // ---- the transform-fused pipelines over a resident batch (include/nflhip.h "transform-fused pipelines"; what the
  // reference's LWE demo does around its transforms, tests/nfllib_demo_main_op.cpp:26-58).  `k` operands are in NTT form
  // and hold either one polynomial (a key shared by the whole batch) or one per element.  Results are bit-identical to
  //     X.set(x); E.set(e); X.ntt_pow_phi(); E.ntt_pow_phi(); *this = X * k + E;          (stream ids taken in that order)
  //     *this = b -+ a * k; this->invntt_pow_invphi();
  // -- the Gaussian polynomials only ever exist as one signed integer per coefficient, the transformed ones not at all.
  template <class Gx, class Ge> void assign_gaussian_fma(Gx const &x, const device_batch &k, Ge const &e) {
    gaussian_fma(nullptr, x, k, e, nullptr, e);
  }
  // *this = NTT(x) * k0 + NTT(e0), out1 = NTT(x) * k1 + NTT(e1): x is drawn and transformed once
  template <class Gx, class G0, class G1>
  void assign_gaussian_fma2(device_batch &out1, Gx const &x, const device_batch &k0, G0 const &e0, const device_batch &k1, G1 const &e1) {
    same_size(out1);
    gaussian_fma(&out1, x, k0, e0, &k1, e1);
  }
  // *this = INTT(b - a * k) (subtract) or INTT(b + a * k); a, b, k in NTT form; *this may be a or b
  void assign_fma_inv(const device_batch &a, const device_batch &k, const device_batch &b, bool subtract) {
    same_size(a);
    same_size(b);
    nflhip_operand oa = {a.d_, 1, NFLHIP_FMT_WORDS}, ok = key_operand(k), ob = {b.d_, 1, NFLHIP_FMT_WORDS};
    detail::check(ctx(), nflhip_fma_inv_dev(ctx(), d_, &oa, &ok, &ob, subtract ? 1 : 0, n_, queue()), "multiply-add + inverse transform");
  }
  // replicate one polynomial over the batch (a key shared by every ciphertext, ...)
  void fill(const P &one) {  // one upload + one broadcast kernel
    void *tmp = nullptr;
    detail::check(ctx(), nflhip_malloc(ctx(), &tmp, sizeof(P)), "device allocation");
    int rc = nflhip_memcpy_h2d(ctx(), tmp, one.cdata(), sizeof(P), queue());
    if (rc == 0) rc = nflhip_broadcast_dev(ctx(), d_, tmp, n_, queue());
    if (rc == 0) rc = nflhip_stream_sync(ctx(), queue());
    nflhip_free(ctx(), tmp);
    detail::check(ctx(), rc, "fill");
  }
  // the same from a resident handle: no host copy at all (a peer-to-peer copy when the batch lives on another device)
  void fill(const poly_p<value_type, P::degree, P::nmoduli> &one) {
    typedef detail::payload<P> payload_type;
    const void *src = static_cast<payload_type *>(one.payload_id())->dev_ro();
    if (ctx() == P::ctx()) {
      detail::check(ctx(), nflhip_broadcast_dev(ctx(), d_, src, n_, queue()), "fill");
      return;
    }
    detail::check(P::ctx(), nflhip_stream_sync(P::ctx(), P::queue()), "fill");  // the handle's pending writes
    void *tmp = nullptr;
    detail::check(ctx(), nflhip_malloc(ctx(), &tmp, sizeof(P)), "device allocation");
    int rc = nflhip_memcpy_peer_dev(ctx(), tmp, P::ctx(), src, sizeof(P), queue());
    if (rc == 0) rc = nflhip_broadcast_dev(ctx(), d_, tmp, n_, queue());
    if (rc == 0) rc = nflhip_stream_sync(ctx(), queue());
    nflhip_free(ctx(), tmp);
    detail::check(ctx(), rc, "fill");
  }
  bool any_equal(const device_batch &o) const { return cmp(o, true); }    // the reference's `a == b`
  bool any_differs(const device_batch &o) const { return cmp(o, false); } // the reference's `a != b`
  // 64-bit digest that composes over shards (nflhip_digest_dev): the digests of the shards of a batch add up to the
  // digest of the batch
  uint64_t digest(size_t first_poly = 0) const {
    uint64_t h = 0;
    detail::check(ctx(), nflhip_digest_dev(ctx(), d_, first_poly, n_, &h, queue()), "digest");
    return h;
  }

 private:
  void same_size(const device_batch &o) const {
    if (o.n_ != n_) throw std::runtime_error("nfl(hip): batch size mismatch");
    if (o.c_ != c_) throw std::runtime_error("nfl(hip): the batches of one operation must live on one device");
  }
  void decompose_sizes(const device_batch &src, int w) const {
    same_device(src);
    const size_t terms = nflhip_decompose_terms(ctx(), w);
    if (terms == 0) throw std::runtime_error("nfl(hip): the digit width is out of range");
    if (n_ != src.n_ * terms) throw std::runtime_error("nfl(hip): a decomposition holds src.size() * terms polynomials");
  }
  void same_device(const device_batch &o) const {
    if (o.c_ != c_) throw std::runtime_error("nfl(hip): the batches of one operation must live on one device");
  }
  void sample(int dist, uint64_t p0, uint64_t p1, const char *what, size_t first_poly, uint64_t stream_id) {
    detail::sampler &s = detail::sampler::get();
    detail::check(ctx(), nflhip_sample_dev(ctx(), d_, first_poly, n_, dist, p0, p1, s.key, stream_id, queue()), what);
  }
  bool cmp(const device_batch &o, bool want_eq) const {
    same_size(o);
    int r = 0;
    detail::check(ctx(), want_eq ? nflhip_any_eq_dev(ctx(), d_, o.d_, n_, &r, queue())
                                 : nflhip_any_neq_dev(ctx(), d_, o.d_, n_, &r, queue()), "compare");
    return r != 0;
  }
  nflhip_operand key_operand(const device_batch &k) const {
    if (k.c_ != c_) throw std::runtime_error("nfl(hip): the batches of one operation must live on one device");
    if (k.n_ != 1 && k.n_ != n_) throw std::runtime_error("nfl(hip): a key operand holds one polynomial or one per element");
    nflhip_operand o = {k.d_, size_t(k.n_ == 1 ? 0 : 1), NFLHIP_FMT_WORDS};
    return o;
  }
  // compact Gaussian polynomials of one call: a grow-only buffer of this batch (its consumers are on the batch's stream)
  void *small_buffer(size_t bytes) {
    if (bytes > small_cap_) {
      if (small_) {
        sync();
        nflhip_free(ctx(), small_);
        small_ = nullptr;
        small_cap_ = 0;
      }
      detail::check(ctx(), nflhip_malloc(ctx(), &small_, bytes), "compact sampler buffer");
      small_cap_ = bytes;
    }
    return small_;
  }
  template <class Gx, class G0, class G1>
  void gaussian_fma(device_batch *out1, Gx const &x, const device_batch &k0, G0 const &e0, const device_batch *k1, G1 const &e1) {
    typedef detail::lazy<P> lazy_t;
    detail::sampler &s = detail::sampler::get();
    const nflhip_gauss *tab[3] = {x.fg_prng->table(ctx()), e0.fg_prng->table(ctx()), out1 ? e1.fg_prng->table(ctx()) : nullptr};
    const uint64_t amp[3] = {x.amplifier, e0.amplifier, out1 ? e1.amplifier : 0};
    const int nx = out1 ? 3 : 2;
    int fmt = NFLHIP_FMT_I8;
    for (int j = 0; j < nx; ++j) fmt = std::max(fmt, (amp[j] >> 32) ? 99 : lazy_t::small_format(tab[j], uint32_t(amp[j])));
    if (fmt > NFLHIP_FMT_I32) {   // samples too wide for a compact format: the operator sequence itself
      const unsigned char fma[] = {0, 1, NFLHIP_EXPR_MUL, 2, NFLHIP_EXPR_ADD};
      device_batch X(n_, c_->device), E(n_, c_->device), K(n_, c_->device);
      X.set(x);
      E.set(e0);
      X.ntt_pow_phi();
      E.ntt_pow_phi();
      const device_batch *kk[2] = {&k0, k1};
      device_batch *oo[2] = {this, out1};
      for (int r = 0; r < (out1 ? 2 : 1); ++r) {
        if (r) {
          E.set(e1);
          E.ntt_pow_phi();
        }
        const device_batch *key = kk[r];
        if (key->n_ == 1) {   // (the expression entry takes dense operands: replicate the key)
          nflhip_operand src = {key->d_, 0, NFLHIP_FMT_WORDS};
          detail::check(ctx(), nflhip_expand_small_dev(ctx(), K.d_, &src, n_, queue()), "key broadcast");
          key = &K;
        }
        const device_batch *ops[] = {&X, key, &E};
        oo[r]->assign_program(fma, sizeof(fma), ops, 3);
      }
      sync();   // (the temporaries die here)
      return;
    }
    const size_t es = fmt == NFLHIP_FMT_I8 ? 1 : fmt == NFLHIP_FMT_I16 ? 2 : 4, each = (n_ * P::degree * es + 255) / 256 * 256;
    char *buf = static_cast<char *>(small_buffer(each * size_t(nx)));
    nflhip_operand xo[3];
    void *dst[3];
    uint64_t sid[3];
    bool one_table = true;
    for (int j = 0; j < nx; ++j) {
      dst[j] = buf + each * size_t(j);
      sid[j] = s.next++;
      one_table &= tab[j] == tab[0];
      xo[j].ptr = dst[j];
      xo[j].stride = 1;
      xo[j].format = fmt;
    }
    if (one_table) {   // the draws of one generator: one launch
      detail::check(ctx(), nflhip_sample_gauss_small_multi_dev(ctx(), dst, size_t(nx), fmt, n_, tab[0], amp, s.key, sid, nullptr, queue()),
                    "set(gaussian), compact");
    } else {
      for (int j = 0; j < nx; ++j)
        detail::check(ctx(), nflhip_sample_gauss_small_dev(ctx(), dst[j], fmt, 0, n_, tab[j], amp[j], s.key, sid[j], queue()), "set(gaussian), compact");
    }
    nflhip_operand ka = key_operand(k0);
    if (out1) {
      nflhip_operand kb = key_operand(*k1);
      detail::check(ctx(), nflhip_fwd_fma2_dev(ctx(), d_, out1->d_, &xo[0], &ka, &xo[1], &kb, &xo[2], n_, queue()), "transform + multiply-add");
    } else {
      detail::check(ctx(), nflhip_fwd_fma_dev(ctx(), d_, &xo[0], &ka, &xo[1], n_, queue()), "transform + multiply-add");
    }
  }
  size_t n_;
  void *d_;
  context_type *c_;
  void *small_ = nullptr;
  size_t small_cap_ = 0;
};

// ---------------------------------------------------------------- batches split over the GPUs of one node
// The reference's callers hold dense arrays of independent polynomials (tests/tools.h:6-17) and loop over them; nothing
// in a loop iteration depends on another (core.hpp:597-599, 610-612, 31-35).  sharded_batch<P> cuts such an array into
// CONTIGUOUS shards, one per GPU (device r of n owns polynomials [first(r), first(r) + count(r)), nflhip_shard_range),
// from ONE process: one context and one stream per device, every operation fans out as one asynchronous call per shard
// (the host thread only enqueues), and there is no data-path collective -- operands are generated in place (the random
// constructors offset their keystream by the shard's first polynomial, so the shards of a batch equal the batch drawn
// on one device), uploaded shard by shard, or scattered once from a batch that lives on one device (peer-to-peer copies,
// one per link).  digest() is the checksum of checksums: the shard digests add up to the digest of the whole batch.
template <class P> class sharded_batch {
 public:
  typedef typename P::value_type value_type;
  typedef device_batch<P> shard_type;
  // all GPUs of the node
  explicit sharded_batch(size_t count) : sharded_batch(count, all_devices()) {}
  sharded_batch(size_t count, std::vector<int> const &devices) : n_(count) {
    if (devices.empty()) throw std::runtime_error("nfl(hip): sharded_batch needs at least one device");
    const int nd = int(devices.size());
    for (int r = 0; r < nd; ++r) {
      size_t f = 0, c = 0;
      detail::check(nullptr, nflhip_shard_range(count, nd, r, &f, &c), "shard_range");
      first_.push_back(f);
      shards_.emplace_back(c, devices[size_t(r)]);
    }
  }
  static std::vector<int> all_devices() {
    std::vector<int> d;
    for (int i = 0, n = device_count(); i < n; ++i) d.push_back(i);
    return d;
  }
  size_t size() const { return n_; }
  size_t shards() const { return shards_.size(); }
  shard_type &shard(size_t r) { return shards_[r]; }
  const shard_type &shard(size_t r) const { return shards_[r]; }
  size_t first(size_t r) const { return first_[r]; }
  size_t count(size_t r) const { return shards_[r].size(); }

  // host array <-> shards: every device moves its own slice (n independent PCIe streams), then one wait for all
  void upload(const P *host) {
    for (size_t r = 0; r < shards(); ++r)
      if (count(r)) detail::check(shards_[r].ctx(), nflhip_memcpy_h2d(shards_[r].ctx(), shards_[r].data(), host[first_[r]].cdata(),
                                                                       shards_[r].bytes(), shards_[r].queue()), "upload");
    sync();
  }
  void download(P *host) const {
    for (size_t r = 0; r < shards(); ++r)
      if (count(r)) detail::check(shards_[r].ctx(), nflhip_memcpy_d2h(shards_[r].ctx(), host[first_[r]].data(), shards_[r].data(),
                                                                       shards_[r].bytes(), shards_[r].queue()), "download");
    sync();
  }
  // a batch resident on ONE device <-> shards: peer-to-peer copies, each on the receiving / sending peer's stream
  void scatter(const shard_type &full) { move(const_cast<shard_type &>(full), true); }
  void gather(shard_type &full) const { const_cast<sharded_batch *>(this)->move(full, false); }

  void sync() const { for (auto &s : shards_) s.sync(); }

  // the batch operations of device_batch, one asynchronous call per shard
  void ntt_pow_phi() { for (auto &s : shards_) if (s.size()) s.ntt_pow_phi(); }
  void invntt_pow_invphi() { for (auto &s : shards_) if (s.size()) s.invntt_pow_invphi(); }
  void assign(int op, const sharded_batch &a, const sharded_batch &b) {
    same_split(a); same_split(b);
    for (size_t r = 0; r < shards(); ++r) if (count(r)) shards_[r].assign(op, a.shards_[r], b.shards_[r]);
  }
  void assign_mul_shoup(const sharded_batch &a, const sharded_batch &b, const sharded_batch &bprime) {
    same_split(a); same_split(b); same_split(bprime);
    for (size_t r = 0; r < shards(); ++r) if (count(r)) shards_[r].assign_mul_shoup(a.shards_[r], b.shards_[r], bprime.shards_[r]);
  }
  void assign_compute_shoup(const sharded_batch &b) {
    same_split(b);
    for (size_t r = 0; r < shards(); ++r) if (count(r)) shards_[r].assign_compute_shoup(b.shards_[r]);
  }
  void assign_polymul(const sharded_batch &a, const sharded_batch &b) {
    same_split(a); same_split(b);
    for (size_t r = 0; r < shards(); ++r) if (count(r)) shards_[r].assign_polymul(a.shards_[r], b.shards_[r]);
  }
  void assign_polymul_ntt(const sharded_batch &a, const sharded_batch &b_ntt) {
    same_split(a); same_split(b_ntt);
    for (size_t r = 0; r < shards(); ++r) if (count(r)) shards_[r].assign_polymul_ntt(a.shards_[r], b_ntt.shards_[r]);
  }
  void assign_automorphism(const sharded_batch &src, uint64_t k, bool ntt_form = false) {
    same_split(src);
    for (size_t r = 0; r < shards(); ++r) if (count(r)) shards_[r].assign_automorphism(src.shards_[r], k, ntt_form);
  }
  template <class Q> void assign_rescale(const sharded_batch<Q> &src, bool ntt_form = false) {  // shard by shard
    if (src.size() != n_ || src.shards() != shards()) throw std::runtime_error("nfl(hip): sharded batches are split differently");
    for (size_t r = 0; r < shards(); ++r)
      if (src.count(r) != count(r) || src.shard(r).device() != shards_[r].device()) throw std::runtime_error("nfl(hip): sharded batches are split differently");
    for (size_t r = 0; r < shards(); ++r) if (count(r)) shards_[r].assign_rescale(src.shard(r), ntt_form);
  }
  void assign_base_convert(const sharded_batch &src, size_t s0, size_t ks, size_t d0, size_t kd, bool centered = false,
                           bool ntt_form = false) {  // whole polynomials per shard
    same_split(src);
    for (size_t r = 0; r < shards(); ++r) {
      if (!count(r)) continue;
      if (ntt_form) shards_[r].assign_base_convert(src.shards_[r], s0, ks, d0, kd, centered, true);
      else shards_[r].assign_base_convert(src.shards_[r], s0, ks, d0, kd, centered);
    }
  }
  template <class Q> void assign_mod_down(const sharded_batch<Q> &src, bool floor = false, bool ntt_form = false) {  // shard by shard
    if (src.size() != n_ || src.shards() != shards()) throw std::runtime_error("nfl(hip): sharded batches are split differently");
    for (size_t r = 0; r < shards(); ++r)
      if (src.count(r) != count(r) || src.shard(r).device() != shards_[r].device()) throw std::runtime_error("nfl(hip): sharded batches are split differently");
    for (size_t r = 0; r < shards(); ++r) {
      if (!count(r)) continue;
      if (ntt_form) shards_[r].assign_mod_down(src.shard(r), floor, true);
      else shards_[r].assign_mod_down(src.shard(r), floor);
    }
  }
  static void assign_automorphisms(sharded_batch *const *outs, const uint64_t *ks, size_t count, const sharded_batch &src,
                                   bool ntt_form = false) {
    if (count > NFLHIP_AUTOMORPHISM_MAX_OUTPUTS) throw std::runtime_error("nfl(hip): too many automorphism outputs");
    for (size_t m = 0; m < count; ++m) src.same_split(*outs[m]);
    for (size_t r = 0; r < src.shards(); ++r) {
      if (!src.count(r)) continue;
      shard_type *d[NFLHIP_AUTOMORPHISM_MAX_OUTPUTS];
      for (size_t m = 0; m < count; ++m) d[m] = &outs[m]->shards_[r];
      shard_type::assign_automorphisms(d, ks, count, src.shards_[r], ntt_form);
    }
  }
  void assign_program(const unsigned char *program, size_t len, const sharded_batch *const *operands, size_t nops) {
    if (nops > NFLHIP_EXPR_MAX_OPERANDS) throw std::runtime_error("nfl(hip): too many operands");
    for (size_t i = 0; i < nops; ++i) same_split(*operands[i]);
    for (size_t r = 0; r < shards(); ++r) {
      if (!count(r)) continue;
      const shard_type *ops[NFLHIP_EXPR_MAX_OPERANDS];
      for (size_t i = 0; i < nops; ++i) ops[i] = &operands[i]->shards_[r];
      shards_[r].assign_program(program, len, ops, nops);
    }
  }
  // in-place generation: ONE keystream for the logical batch, every shard reads its own positions of it
  void set(uniform const &u) {
    const uint64_t sid = u.seeded ? 0 : detail::sampler::get().next++;
    for (size_t r = 0; r < shards(); ++r) {
      if (!count(r)) continue;
      if (u.seeded) shards_[r].set(u, first_[r]);
      else shards_[r].set_at(u, first_[r], sid);
    }
  }
  void set(non_uniform const &m) { set_shards(m); }
  void set(ZO_dist const &m) { set_shards(m); }
  void set(hwt_dist const &m) { set_shards(m); }
  template <class in_class, unsigned _lu_depth> void set(gaussian<in_class, value_type, _lu_depth> const &m) { set_shards(m); }
  // one polynomial replicated over every shard
  void fill(const P &one) { for (auto &s : shards_) if (s.size()) s.fill(one); }

  // the reference's `==` / `!=` over the whole array ("any lane", ops.hpp:81-117): any shard
  bool any_equal(const sharded_batch &o) const {
    same_split(o);
    bool r = false;
    for (size_t k = 0; k < shards(); ++k) if (count(k)) r = shards_[k].any_equal(o.shards_[k]) || r;
    return r;
  }
  bool any_differs(const sharded_batch &o) const {
    same_split(o);
    bool r = false;
    for (size_t k = 0; k < shards(); ++k) if (count(k)) r = shards_[k].any_differs(o.shards_[k]) || r;
    return r;
  }
  // per-shard digests (positions counted in the WHOLE batch) and their sum = the digest of the batch on one device
  std::vector<uint64_t> digests() const {
    std::vector<uint64_t> d(shards());
    for (size_t r = 0; r < shards(); ++r) d[r] = count(r) ? shards_[r].digest(first_[r]) : 0;
    return d;
  }
  uint64_t digest() const {
    uint64_t s = 0;
    for (uint64_t d : digests()) s += d;
    return s;
  }

 private:
  template <class D> void set_shards(D const &m) {
    const uint64_t sid = detail::sampler::get().next++;
    for (size_t r = 0; r < shards(); ++r) if (count(r)) shards_[r].set_at(m, first_[r], sid);
  }
  void same_split(const sharded_batch &o) const {
    if (o.n_ != n_ || o.shards() != shards()) throw std::runtime_error("nfl(hip): batch size mismatch");
    for (size_t r = 0; r < shards(); ++r)
      if (o.shards_[r].ctx() != shards_[r].ctx()) throw std::runtime_error("nfl(hip): the batches of one operation must be split over the same devices");
  }
  void move(shard_type &full, bool to_shards) {
    if (full.size() != n_) throw std::runtime_error("nfl(hip): batch size mismatch");
    std::vector<nflhip_ctx *> ctxs;
    std::vector<void *> ptrs, streams;
    int root = -1;
    for (size_t r = 0; r < shards(); ++r) {
      ctxs.push_back(shards_[r].ctx());
      ptrs.push_back(shards_[r].data());
      streams.push_back(shards_[r].queue());
      if (shards_[r].ctx() == full.ctx()) root = int(r);
    }
    if (root < 0) throw std::runtime_error("nfl(hip): the whole batch must live on one of the shards' devices");
    const int rc = to_shards ? nflhip_scatter_local_dev(ctxs.data(), int(ctxs.size()), ptrs.data(), root, full.data(), n_, streams.data())
                             : nflhip_gather_local_dev(ctxs.data(), int(ctxs.size()), full.data(), root, ptrs.data(), n_, streams.data());
    detail::check(full.ctx(), rc, to_shards ? "scatter" : "gather");
  }
  size_t n_;
  std::vector<size_t> first_;
  std::vector<shard_type> shards_;
};

}  // namespace nfl
#endif  // NFL_HIP_BATCH_HPP
