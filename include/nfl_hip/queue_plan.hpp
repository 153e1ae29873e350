// nfl_hip/queue_plan.hpp -- part of the drop-in header; include <nfl_hip/nfl.hpp> (or the reference's names under include/nfl*).
// planning a run of the deferred queue: the recorded operation, what it reads and writes, its signature, transform fusion,
// dependency levelling, grouping and the stride runs.  Everything here looks at records and per-pin arrays only: no thread, no
// lock, no launch; what has to be asked of the backend is passed in (queue.hpp: lazy<P>::small_format, fusion_on).
#ifndef NFL_HIP_QUEUE_PLAN_HPP
#define NFL_HIP_QUEUE_PLAN_HPP
#ifndef NFL_HIP_NFL_HPP
#error "include <nfl_hip/nfl.hpp>: the parts depend on each other in its order"
#endif
namespace nfl {
namespace detail {
struct queue_kinds {
  // K_FWD_FMA / K_FMA_INV / K_NOP are never recorded: a queue run rewrites recorded sequences into them (plan<P>::fuse)
  enum kind_t { K_EVAL = 0, K_NTT_FWD, K_NTT_INV, K_SAMPLE, K_GAUSS, K_FILL, K_FWD_FMA, K_FMA_INV, K_NOP };
  static constexpr int max_in = 4;  // expressions with more distinct handle operands are launched at once, not recorded
};

template <class P> struct plan : queue_kinds {
  typedef payload<P> pay_t;
  static constexpr size_t chunk = pay_t::ctx_t::chunk_bytes;
  // One recorded operation: 120 bytes, trivially destructible.  The payloads it names are kept alive by ONE reference per
  // payload and queue run (lazy<P>::pins), not one per mention -- a loop's temporaries are mentioned three times each.
  struct op {
    pay_t *out;
    union {
      struct {
        pay_t *in[max_in];
        unsigned char code[NFLHIP_EXPR_MAX_LEN];
      } e;          // K_EVAL (the transforms use out only)
      struct {
        uint64_t p0, p1, sid;
        const nflhip_gauss *tab;
        int dist;
      } s;          // K_SAMPLE, K_GAUSS, K_FILL
      struct {
        pay_t *in[max_in];     // the key operands k0 [, k1] (same place as e.in: for_each_pin reads them through it)
        pay_t *out2;           // second result (out1 = NTT(x) * k1 + NTT(e1)), or nullptr
        uint64_t sid[3];       // stream ids of the Gaussian polynomials x, e0, e1
        uint32_t amp[3];       // their amplifiers
        unsigned out2_pin;
        const nflhip_gauss *tab;
      } f;          // K_FWD_FMA
    };
    unsigned char kind, nin, len;
    unsigned char post;   // 0, or K_NTT_FWD / K_NTT_INV: the result is transformed in place right after (a transform recorded on
                          // a value nothing had read since this operation produced it joins the operation instead of becoming a record)
    // Where the run's references to `out` and to the inputs sit in its pin list.  A queue run works on THESE: whatever it keeps
    // per value (buffer, levels, last writer) lives in arrays of its own, indexed by pin -- it never touches a payload, whose
    // cache lines stay with the recording thread (the first version of the queue's thread wrote its levelling scratch into the
    // payloads: the recording thread then fetched every line back from the other core when it retired the run, 1.5 us per LWE
    // encryption, 2.5 times slower than no thread at all).
    unsigned out_pin, in_pin[max_in];
  };
  // ---- what an operation reads and writes: on_read(payload, pin) for every value it reads, then on_write(payload, pin) for
  // every value it writes (`pin` is the record's own slot: callers that pin payloads write it).  An in-place transform reads and
  // writes `out`; the second result of K_FWD_FMA is a second write; K_NOP (its work moved into a fused operation) is nothing.
  // The fusion's def/use pass, the levelling, mentions() and the recording side's pinning are all written on top of this.
  template <class O, class R, class W> static void for_each_pin(O &o, R on_read, W on_write) {
    if (o.kind == K_NOP) return;
    for (int j = 0; j < o.nin; ++j) on_read(o.e.in[j], o.in_pin[j]);
    if (o.kind == K_NTT_FWD || o.kind == K_NTT_INV) on_read(o.out, o.out_pin);
    on_write(o.out, o.out_pin);
    if (o.kind == K_FWD_FMA && o.f.out2) on_write(o.f.out2, o.f.out2_pin);
  }
  static bool mentions(const op &o, unsigned pin) {
    bool hit = false;
    for_each_pin(o, [&](pay_t *, const unsigned &k) { hit |= k == pin; }, [&](pay_t *, const unsigned &k) { hit |= k == pin; });
    return hit;
  }
  // ---- signature: everything a launch takes from its first member.  Two operations may share a launch when their keys are
  // equal; the groups are found by the key's hash and confirmed by comparing the keys.
  struct sig { uint64_t w[5]; };
  static_assert(NFLHIP_EXPR_MAX_LEN <= 24, "the program is kept as three words");
  static sig signature(const op &o) {
    sig k = {{uint64_t(o.kind) | (uint64_t(o.post) << 8), 0, 0, 0, 0}};
    if (o.kind == K_EVAL) {
      std::memcpy(&k.w[1], o.e.code, size_t(o.len));
      k.w[4] = (uint64_t(o.len) << 8) | uint64_t(o.nin);
    } else if (o.kind == K_SAMPLE || o.kind == K_GAUSS) {
      k.w[1] = uint64_t(o.s.dist);
      k.w[2] = o.s.p0;
      k.w[3] = o.s.p1;
      k.w[4] = uint64_t(reinterpret_cast<uintptr_t>(o.s.tab));
    } else if (o.kind == K_FILL) {
      k.w[1] = o.s.sid;
    } else if (o.kind == K_FWD_FMA) {
      k.w[1] = uint64_t(reinterpret_cast<uintptr_t>(o.f.tab));
      k.w[2] = (uint64_t(o.f.amp[0]) << 32) | o.f.amp[1];
      k.w[3] = (uint64_t(o.f.amp[2]) << 8) | o.nin;
    } else if (o.kind == K_FMA_INV) {
      k.w[1] = o.e.code[0];
    }
    return k;
  }
  static bool same_signature(const sig &a, const sig &b) { return std::memcmp(&a, &b, sizeof(sig)) == 0; }
  static uint64_t mix(uint64_t h, uint64_t v) {  // (one multiply-xorshift round per 64-bit word: the signatures are a few words)
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
  }
  static uint64_t hash(const sig &k) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (int j = 0; j < 5; ++j) h = mix(h, k.w[j]);
    return h;
  }
  // ---- transform fusion.  Code written against the reference transforms, combines, transforms back:
  //        u.ntt_pow_phi(); e.ntt_pow_phi(); r = u * key + e;          out = rb - ra * s; out.invntt_pow_invphi();
  // (tests/nfllib_demo_main_op.cpp:26-58).  When this context runs such a sequence as ONE kernel (nflhip_has_fused_kernels),
  // a queue run rewrites what it recorded before it levels it:
  //   * K_GAUSS x, K_NTT_FWD x, K_GAUSS e, K_NTT_FWD e, K_EVAL r = x * k + e (either operand order; a second K_EVAL on the
  //     same x with its own k, e joins) -> K_FWD_FMA, provided nothing else reads the sampled or transformed x / e and
  //     their handles are gone (the queue holds the last reference): those polynomials then never exist in HBM -- the
  //     samplers write one byte per coefficient (nflhip_sample_gauss_small_seq_dev) and the kernel transforms in registers;
  //   * K_EVAL t = c +- a * b, K_NTT_INV t with nothing reading t in between -> K_FMA_INV.
  // Results are bit-identical to the operator-by-operator run.  NFL_HIP_NO_FUSION=1 switches the rewriting off.
  //
  // c +- a * b as a 5-byte postfix program over three distinct operands: {a, b, c, subtract}, or false.  A record that
  // carries a joined transform (op::post, lazy<P>::join_transform) is NOT that expression: its result is the transformed
  // value, and a rewrite that took only the expression would drop the transform.  The one place that models a joined
  // transform -- the expression followed by its own inverse transform -- asks for it by name (`joined`).
  static bool parse_fma(const op &o, int &a, int &b, int &c, bool &sub, unsigned char joined = 0) {
    if (o.kind != K_EVAL || o.len != 5 || o.nin != 3 || o.post != joined) return false;
    const unsigned char *q = o.e.code;
    if (q[0] < 3 && q[1] < 3 && q[2] == NFLHIP_EXPR_MUL && q[3] < 3 && q[4] == NFLHIP_EXPR_ADD) {            // a b * c +
      a = q[0]; b = q[1]; c = q[3]; sub = false;
    } else if (q[0] < 3 && q[1] < 3 && q[2] < 3 && q[3] == NFLHIP_EXPR_MUL && (q[4] == NFLHIP_EXPR_ADD || q[4] == NFLHIP_EXPR_SUB)) {  // c a b * +-
      c = q[0]; a = q[1]; b = q[2]; sub = q[4] == NFLHIP_EXPR_SUB;
    } else {
      return false;
    }
    return a != b && a != c && b != c;
  }
  // the narrowest compact format that holds every sample of a table times an amplifier (NFLHIP_FMT_I8 / I16 / I32; 99 = none)
  typedef int (*format_query)(const nflhip_gauss *, uint32_t);
  // definitions and uses of one run's records, as recorded: prev[i] = the operation that wrote ops[i].out before i (what an
  // in-place transform reads), def[i][j] = the one that wrote input j of an expression; uses[d] = reads of the value operation
  // d wrote; -1 = from before this run.  fw, per pin: the recorded operation that last wrote the value.
  struct defuse {
    std::vector<int> prev, uses, def;
    std::vector<int> &fw;
    const std::vector<unsigned char> &dead;
    bool any_fwd, any_inv;
    defuse(const std::vector<op> &ops, std::vector<int> &fw_, const std::vector<unsigned char> &dead_)
        : prev(ops.size(), -1), uses(ops.size(), 0), def(ops.size() * 3, -1), fw(fw_), dead(dead_), any_fwd(false), any_inv(false) {
      fw.assign(dead.size(), -1);
      for (int i = 0; i < int(ops.size()); ++i) {
        const op &o = ops[size_t(i)];
        int j = 0;
        auto on_read = [&](pay_t *, const unsigned &k) {
          if (o.kind == K_EVAL && j < 3) def[size_t(i) * 3 + size_t(j)] = fw[k];
          ++j;
          if (fw[k] >= 0) ++uses[size_t(fw[k])];
        };
        // (one write per record: the kinds with two are made by the fusion)
        for_each_pin(o, on_read, [&](pay_t *, const unsigned &k) { prev[size_t(i)] = fw[k]; fw[k] = i; });
        any_fwd |= o.kind == K_NTT_FWD || o.post == K_NTT_FWD;
        any_inv |= o.kind == K_NTT_INV || o.post == K_NTT_INV;
      }
    }
    // the value an operation wrote is still its payload's at the end of the run: only fusable away when no handle is left
    bool dead_after(const std::vector<op> &ops, int d) const {
      const unsigned k = ops[size_t(d)].out_pin;
      return fw[k] != d || dead[k] != 0;   // (this run's pin was the last reference when the run was taken: no handle, no later record)
    }
    // a sampled-and-transformed polynomial nobody else sees: -> index of its K_GAUSS record, or -1
    int gauss_chain(const std::vector<op> &ops, int dn, int want_uses, format_query small_format) const {
      if (dn < 0 || uses[size_t(dn)] != want_uses || !dead_after(ops, dn)) return -1;
      int g = dn;   // the transform joined its constructor's record (post), or is a record of its own after it
      if (ops[size_t(dn)].kind == K_NTT_FWD) {
        g = prev[size_t(dn)];
        if (g < 0 || ops[size_t(g)].post != 0 || uses[size_t(g)] != 1) return -1;   // (post: the constructor's record already carries one transform; this would be the second)
      } else if (ops[size_t(dn)].post != K_NTT_FWD) {
        return -1;
      }
      const op &s = ops[size_t(g)];
      if (s.kind != K_GAUSS || (s.s.p1 >> 32) != 0 || small_format(s.s.tab, uint32_t(s.s.p1)) > NFLHIP_FMT_I32) return -1;
      return g;
    }
  };
  // t becomes in[c] +- in[a] * in[b] of expression e, followed by the inverse transform (t may be e itself)
  static void to_fma_inv(op &t, const op &e, int a, int b, int c, bool sub) {
    pay_t *const p[3] = {e.e.in[c], e.e.in[a], e.e.in[b]};
    const unsigned k[3] = {e.in_pin[c], e.in_pin[a], e.in_pin[b]};
    t.kind = K_FMA_INV;
    t.post = 0;
    t.nin = 3;
    t.len = 1;
    for (int j = 0; j < 3; ++j) {
      t.e.in[j] = p[j];
      t.in_pin[j] = k[j];
    }
    t.e.code[0] = sub ? 1 : 0;
  }
  static size_t fuse_inverse(std::vector<op> &ops, const defuse &du) {
    size_t fused = 0;
    for (int i = 0; i < int(ops.size()); ++i) {
      op &t = ops[size_t(i)];
      int a, b, c;
      bool sub;
      if (parse_fma(t, a, b, c, sub, K_NTT_INV)) {   // the transform joined the expression's record: rewrite in place
        to_fma_inv(t, t, a, b, c, sub);
        ++fused;
        continue;
      }
      if (t.kind != K_NTT_INV) continue;
      const int d = du.prev[size_t(i)];
      if (d < 0 || i - d > 4 || du.uses[size_t(d)] != 1 || !parse_fma(ops[size_t(d)], a, b, c, sub)) continue;
      op &e = ops[size_t(d)];
      bool clean = true;   // nothing between the two rewrites an operand (the fused operation reads them at i, not at d)
      for (int k = d + 1; k < i && clean; ++k)
        clean = ops[size_t(k)].kind == K_NOP || (ops[size_t(k)].out_pin != e.in_pin[0] && ops[size_t(k)].out_pin != e.in_pin[1] && ops[size_t(k)].out_pin != e.in_pin[2]);
      if (!clean) continue;
      to_fma_inv(t, e, a, b, c, sub);
      e.kind = K_NOP;
      ++fused;
    }
    return fused;
  }
  // forward: candidates per transformed x (an expression names it once; a second expression on the same x joins)
  struct cand { int i, xs, ks, es, gx, ge; };
  // the record of c0 (and of c1, the second expression on the same x, if any) becomes ONE K_FWD_FMA at the later one's place
  static void to_fwd_fma(std::vector<op> &ops, const defuse &du, const cand &c0, const cand *c1) {
    const op e0 = ops[size_t(c0.i)];
    op &t = ops[size_t(c1 ? c1->i : c0.i)];
    const op e1 = t;
    t.kind = K_FWD_FMA;
    t.out = e0.out;
    t.out_pin = e0.out_pin;
    t.nin = c1 ? 2 : 1;
    t.len = 0;
    t.f.in[0] = e0.e.in[c0.ks];
    t.f.in[1] = c1 ? e1.e.in[c1->ks] : nullptr;
    t.f.in[2] = t.f.in[3] = nullptr;
    t.in_pin[0] = e0.in_pin[c0.ks];
    t.in_pin[1] = c1 ? e1.in_pin[c1->ks] : 0;
    t.f.out2 = c1 ? e1.out : nullptr;
    t.f.out2_pin = c1 ? e1.out_pin : 0;
    t.f.tab = ops[size_t(c0.gx)].s.tab;
    const int draws[3] = {c0.gx, c0.ge, c1 ? c1->ge : -1};   // x, e0, e1
    for (int j = 0; j < 3; ++j) {
      t.f.sid[j] = draws[j] >= 0 ? ops[size_t(draws[j])].s.sid : 0;
      t.f.amp[j] = draws[j] >= 0 ? uint32_t(ops[size_t(draws[j])].s.p1) : 0;
    }
    // the records the fused operation stands for
    const int gone[] = {c0.gx, du.def[size_t(c0.i) * 3 + size_t(c0.xs)], c0.ge, du.def[size_t(c0.i) * 3 + size_t(c0.es)], c1 ? c0.i : -1,
                        c1 ? c1->ge : -1, c1 ? du.def[size_t(c1->i) * 3 + size_t(c1->es)] : -1};
    for (int g : gone)
      if (g >= 0) ops[size_t(g)].kind = K_NOP;
  }
  static size_t fuse_forward(std::vector<op> &ops, const defuse &du, format_query small_format) {
    std::vector<cand> cands;
    for (int i = 0; i < int(ops.size()); ++i) {
      int a, b, c;
      bool sub;
      if (!parse_fma(ops[size_t(i)], a, b, c, sub) || sub) continue;
      for (int turn = 0; turn < 2; ++turn) {
        const int xs = turn ? b : a, ks = turn ? a : b;
        const int dx = du.def[size_t(i) * 3 + size_t(xs)], de = du.def[size_t(i) * 3 + size_t(c)];
        if (dx < 0 || de < 0 || dx == de) continue;
        const int ux = du.uses[size_t(dx)];
        if (ux != 1 && ux != 2) continue;
        const int gx = du.gauss_chain(ops, dx, ux, small_format), ge = du.gauss_chain(ops, de, 1, small_format);
        if (gx < 0 || ge < 0 || ops[size_t(gx)].s.tab != ops[size_t(ge)].s.tab) continue;
        cands.push_back(cand{i, xs, ks, c, gx, ge});
        break;
      }
    }
    size_t fused = 0;
    for (size_t q = 0; q < cands.size(); ++q) {
      const cand &c0 = cands[q];
      if (c0.i < 0) continue;
      const int dx = du.def[size_t(c0.i) * 3 + size_t(c0.xs)];
      cand *c1 = nullptr;
      if (du.uses[size_t(dx)] == 2) {   // the other reader of NTT(x) must be a candidate too, close by, and independent of this one
        for (size_t r = q + 1; r < cands.size() && !c1; ++r)
          if (cands[r].i >= 0 && du.def[size_t(cands[r].i) * 3 + size_t(cands[r].xs)] == dx) c1 = &cands[r];
        if (!c1 || c1->i - c0.i > 4) continue;
        const op &e0 = ops[size_t(c0.i)], &e1 = ops[size_t(c1->i)];
        bool clean = e1.in_pin[c1->ks] != e0.out_pin && e1.out_pin != e0.out_pin;   // (the fused operation writes both results at e1's place)
        for (int k = c0.i + 1; k < c1->i && clean; ++k)
          clean = !mentions(ops[size_t(k)], e0.out_pin) && (ops[size_t(k)].kind == K_NOP || ops[size_t(k)].out_pin != e0.in_pin[c0.ks]);
        if (!clean) continue;
      }
      to_fwd_fma(ops, du, c0, c1);
      if (c1) c1->i = -1;
      ++fused;
    }
    return fused;
  }
  // rewrites the records of one run (fw: per-pin scratch; dead: per pin, whether the run holds the last reference) and adds the
  // numbers of forward / inverse sequences it rewrote to the two counters
  template <class N> static void fuse(std::vector<op> &ops, std::vector<int> &fw, const std::vector<unsigned char> &dead, format_query small_format,
                                      N &fused_fwd, N &fused_inv) {
    const defuse du(ops, fw, dead);
    if (du.any_inv) fused_inv += fuse_inverse(ops, du);
    if (du.any_fwd) fused_fwd += fuse_forward(ops, du, small_format);
  }
  // ---- levels: lvl[i] = the level of operation i (-1: K_NOP) such that everything inside a level is independent; wlev / rlev,
  // per pin: the last level that writes / reads the value
  static void level(const std::vector<op> &ops, std::vector<int> &wlev, std::vector<int> &rlev, size_t npins, std::vector<int> &lvl) {
    wlev.assign(npins, -1);
    rlev.assign(npins, -1);
    lvl.assign(ops.size(), -1);
    for (size_t i = 0; i < ops.size(); ++i) {
      const op &o = ops[i];
      if (o.kind == K_NOP) continue;   // its work moved into a fused operation
      int L = 0;
      for_each_pin(o, [&](pay_t *, const unsigned &k) { L = std::max(L, wlev[k] + 1); },
                   [&](pay_t *, const unsigned &k) { L = std::max(L, std::max(wlev[k], rlev[k]) + 1); });
      lvl[i] = L;
      for_each_pin(o, [&](pay_t *, const unsigned &k) { rlev[k] = std::max(rlev[k], L); }, [&](pay_t *, const unsigned &k) { wlev[k] = L; });
    }
  }
  // ---- groups: (level, signature) -> operations in program order.  A loop produces a handful of distinct signatures, so a
  // linear table of the ones seen (hash of the key, plus the level) beats a map.  `order`: the groups level by level (inside a
  // level the order is irrelevant: they are independent)
  struct group { int level; uint64_t hash; sig key; std::vector<size_t> idx; };
  static void group_by_signature(const std::vector<op> &ops, const std::vector<int> &lvl, std::vector<group> &groups, std::vector<size_t> &order) {
    for (size_t i = 0; i < ops.size(); ++i) {
      if (ops[i].kind == K_NOP) continue;
      const sig key = signature(ops[i]);
      const uint64_t h = hash(key);
      size_t g = groups.size();
      for (size_t k = groups.size(); k-- > 0;)   // (recent groups first: neighbouring operations repeat)
        if (groups[k].level == lvl[i] && groups[k].hash == h && same_signature(groups[k].key, key)) { g = k; break; }
      if (g == groups.size()) {
        groups.push_back(group{lvl[i], h, key, std::vector<size_t>()});
        groups.back().idx.reserve(ops.size() / 4 + 1);
      }
      groups[g].idx.push_back(i);
    }
    order.resize(groups.size());
    for (size_t g = 0; g < order.size(); ++g) order[g] = g;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return groups[x].level < groups[y].level; });
  }
  // A loop body that draws several polynomials of one distribution (e1, e2 of an encryption) interleaves their
  // stream ids: k+1, k+2, k+4, k+5, ...  Find the period of the id differences and regroup the operations into
  // that many arithmetic progressions, each of which then gets its own dense array of buffers and is one launch.
  static void regroup_periodic(const std::vector<op> &ops, std::vector<size_t> &idx) {
    for (size_t period = 2; period <= 8 && period * 2 <= idx.size(); ++period) {
      bool periodic = true, constant = true;
      for (size_t i = 0; i + 1 < idx.size() && periodic; ++i) {
        const uint64_t d = ops[idx[i + 1]].s.sid - ops[idx[i]].s.sid;
        if (i + 1 + period < idx.size()) periodic = d == ops[idx[i + 1 + period]].s.sid - ops[idx[i + period]].s.sid;
        constant &= d == ops[idx[1]].s.sid - ops[idx[0]].s.sid;
      }
      if (constant) return;
      if (periodic) {
        std::vector<size_t> re;
        for (size_t r = 0; r < period; ++r)
          for (size_t i = r; i < idx.size(); i += period) re.push_back(idx[i]);
        idx.swap(re);
        return;
      }
    }
  }
  // Operands that are one polynomial for (almost) the whole group split it: a "key" slot holds one of a few polynomials
  // throughout the group (at most 8, and at most every eighth operation a new one); each combination of keys becomes its own
  // sub-group, whose other operands then advance by strides
  struct subgroup { unsigned key[NFLHIP_EXPR_MAX_OPERANDS]; std::vector<size_t> idx; };   // (keys by pin; ~0u: not a key slot)
  static void split_by_keys(const std::vector<op> &ops, const std::vector<size_t> &idx, int nin, std::vector<subgroup> &sub) {
    bool keyslot[NFLHIP_EXPR_MAX_OPERANDS];
    const size_t cap = std::min<size_t>(idx.size() / 8 + 1, 8);
    for (int j = 0; j < nin; ++j) {
      unsigned seen[8];
      size_t ns = 0;
      bool few = idx.size() >= 2;
      for (size_t i : idx) {
        if (!few) break;
        const unsigned p = ops[i].in_pin[j];
        size_t k = ns;
        while (k-- > 0 && seen[k] != p) {}
        if (k == size_t(-1)) {
          if (ns == cap) few = false;
          else seen[ns++] = p;
        }
      }
      keyslot[j] = few && ns < idx.size();
    }
    for (size_t i : idx) {
      unsigned key[NFLHIP_EXPR_MAX_OPERANDS];
      for (int j = 0; j < nin; ++j) key[j] = keyslot[j] ? ops[i].in_pin[j] : ~0u;
      size_t g = sub.size();
      for (size_t k = sub.size(); k-- > 0;)
        if (std::equal(key, key + nin, sub[k].key)) { g = k; break; }
      if (g == sub.size()) {
        sub.emplace_back();
        std::copy(key, key + nin, sub.back().key);
      }
      sub[g].idx.push_back(i);
    }
  }
  // by destination address (program order among equals); a loop's results already are in that order.  D, per pin: the buffer
  static void sort_by_result(const std::vector<op> &ops, std::vector<size_t> &idx, const std::vector<void *> &D) {
    bool sorted = true;
    for (size_t k = 1; k < idx.size() && sorted; ++k) sorted = !(D[ops[idx[k]].out_pin] < D[ops[idx[k - 1]].out_pin]);
    if (!sorted) std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return D[ops[x].out_pin] < D[ops[y].out_pin]; });
  }
  // ---- runs.  A run is ONE launch: members idx[a .. b) whose `nres` result buffers (out [, out2]) advance by one constant
  // positive number of chunks -- exactly one where the entry point writes `dense` results --, whose `nin` operands each advance
  // by a constant number of chunks (0: a key) and whose `nsid` stream ids each advance by a constant difference.  -> b, and
  // the strides in chunks (as the first step set them; of a run of one: result 1, everything else 0)
  struct strides { size_t out, in[NFLHIP_EXPR_MAX_OPERANDS]; uint64_t sid[3]; };
  static unsigned result_pin(const op &o, int j) { return j ? o.f.out2_pin : o.out_pin; }
  static uint64_t stream_id(const op &o, int j) { return o.kind == K_FWD_FMA ? o.f.sid[j] : o.s.sid; }
  static size_t extend_run(const std::vector<op> &ops, const std::vector<size_t> &idx, size_t a, const std::vector<void *> &D, int nres,
                           int nin, int nsid, bool dense, strides &s) {
    s = strides();
    s.out = 1;
    size_t b = a + 1;
    for (; b < idx.size(); ++b) {
      const op &prev = ops[idx[b - 1]], &cur = ops[idx[b]];
      const bool first = b == a + 1;
      bool ok = true;
      for (int j = 0; j < nres && ok; ++j) {
        const ptrdiff_t d = static_cast<char *>(D[result_pin(cur, j)]) - static_cast<char *>(D[result_pin(prev, j)]);
        if (d <= 0 || d % ptrdiff_t(chunk) || (dense && size_t(d) != chunk)) ok = false;
        else if (first && j == 0) s.out = size_t(d) / chunk;
        else if (size_t(d) != s.out * chunk) ok = false;
      }
      for (int j = 0; j < nin && ok; ++j) {
        const ptrdiff_t d = static_cast<char *>(D[cur.in_pin[j]]) - static_cast<char *>(D[prev.in_pin[j]]);
        if (d < 0 || d % ptrdiff_t(chunk)) ok = false;
        else if (first) s.in[j] = size_t(d) / chunk;
        else if (size_t(d) != s.in[j] * chunk) ok = false;
      }
      for (int j = 0; j < nsid && ok; ++j) {
        const uint64_t d = stream_id(cur, j) - stream_id(prev, j);
        if (first) s.sid[j] = d;
        else if (d != s.sid[j]) ok = false;
      }
      if (!ok) break;
    }
    return b;
  }
  // ascending order for addresses that usually are `period` interleaved ascending sequences already (a loop body that
  // transforms u, e1, e2 -- each kind a dense array of its own -- yields u0 e1_0 e2_0 u1 e1_1 e2_1 ...): merged in O(n)
  static void sort_interleaved(std::vector<char *> &v) {
    if (std::is_sorted(v.begin(), v.end())) return;
    for (size_t period = 2; period <= 8 && period * 2 <= v.size(); ++period) {
      bool ok = true;
      for (size_t i = period; i < v.size() && ok; ++i) ok = !(v[i] < v[i - period]);
      if (!ok) continue;
      std::vector<char *> out;
      out.reserve(v.size());
      for (size_t r = 0; r < period; ++r) {
        const size_t mid = out.size();
        for (size_t i = r; i < v.size(); i += period) out.push_back(v[i]);
        std::inplace_merge(out.begin(), out.begin() + ptrdiff_t(mid), out.end());
      }
      v.swap(out);
      return;
    }
    std::sort(v.begin(), v.end());
  }
};
}  // namespace detail
}  // namespace nfl
#endif  // NFL_HIP_QUEUE_PLAN_HPP
