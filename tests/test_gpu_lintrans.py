"""GPU: slot linear transforms (include/nflhip.h "slot linear transforms"; nfllib_amd/csrc/kernels_lintrans.hip and the plans of
api.hip).  Both plans and the default, both mod-up modes and both roundings, word for word against tests/lintrans_util.py
lintrans_rns: the header's definition on Python integers between the CPU oracle's transforms.  No tolerance anywhere.  The inputs
are those of tests/test_gpu_rotate.py (c1 planted per digit with the edge values, the centred band, every y_i = p_i - 1; two random
keys); the diagonals are random canonical words with 0 and p - 1 planted.  The restatement works polynomial by polynomial, so it is
computed once per shape, mode and term list on the planted batch of three and indexed for the other batch sizes."""
import ctypes as C

import numpy as np
import pytest

import baseconv_util as B
from lintrans_util import lintrans_rns
from rotate_util import add_rows
from test_gpu_rotate import MODES, PICK, case, rotations

pytestmark = pytest.mark.gpu

PLANS = ("sequence", "hoisted", None)
_W, _MEMO = {}, {}


def diagonals(e):
    """16 diagonals [nm, n] over all nm moduli"""
    key = (e.limb_bits, e.degree, e.nmoduli)
    if key not in _W:
        ws = [B.random_batch(e.P, e.degree, 1, e.np_dtype, 300 + t)[0] for t in range(16)]
        pm1 = np.array([int(p) - 1 for p in e.P], dtype=e.np_dtype)
        ws[0][:, :2] = pm1[:, None]
        ws[1][:, -1] = 0
        for w in ws:
            w.setflags(write=False)
        _W[key] = ws
    return _W[key]


def terms_of(n, count, unkeyed=()):
    """(ks, index of the key or None) per term: the rotations of tests/test_gpu_rotate.py, the terms listed in `unkeyed` turned
    into the unrotated diagonal (k = 1, no key)"""
    ks, which = rotations(n, count)
    ks, which = list(ks), list(which)
    for m in unkeyed:
        ks[m], which[m] = 1, None
    return ks, which


def setup(e, orc, ok, K, alpha, seed=3, polys=3):
    c0, c1, keys, _ = case(e, orc, ok, K, alpha, seed=seed, polys=polys)
    ws = diagonals(e)

    def want(centered, floor, ks, which, with_c0=True, pick=None):
        memo = _MEMO.setdefault((e.limb_bits, e.degree, e.nmoduli, K, alpha, seed, polys, centered), {})
        r = lintrans_rns(c0 if with_c0 else None, c1, [None if i is None else keys[i] for i in which], ws[:len(ks)], ks, e.P, K, alpha,
                         centered, floor, orc, ok, memo=memo)
        return r if pick is None else (r[0][pick], r[1][pick])
    return c0, c1, keys, ws, want


def run(e, dc0, dc1, dkeys, dws, ks, which, K, alpha, **kw):
    return e.linear_transform_ntt(dc0, dc1, [None if i is None else dkeys[i] for i in which], dws[:len(ks)], ks, K, alpha, **kw)


def same(e, got, want):
    return all(np.array_equal(e.to_host(got[c]).reshape(want[c].shape), want[c]) for c in (0, 1))


def check(e, orc, ok, K, alpha, modes, combos, plans=PLANS, unkeyed=()):
    c0, c1, keys, ws, want = setup(e, orc, ok, K, alpha)
    dkeys, dws = [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    for count, batch in combos:
        ks, which = terms_of(e.degree, count, [m for m in unkeyed if m < count])
        pick = PICK[batch]
        dc0, dc1 = e.to_device(c0[pick]), e.to_device(c1[pick])
        for centered, floor in modes:
            w = want(centered, floor, ks, which, pick=pick)
            for plan in plans:
                got = run(e, dc0, dc1, dkeys, dws, ks, which, K, alpha, centered=centered, floor=floor, plan=plan)
                assert got[0].shape == dc1.shape and got[1].shape == dc1.shape
                assert same(e, got, w), (K, alpha, count, batch, centered, floor, plan)
        assert np.array_equal(e.to_host(dc0), c0[pick]) and np.array_equal(e.to_host(dc1), c1[pick])     # the inputs are unchanged
    assert all(np.array_equal(e.to_host(d), h) for d, h in zip(dkeys + dws, keys + ws))


def test_every_plan_every_mode_every_count_and_batch(engine_factory, oracle_factory):
    """u64/64/5, K 2, alpha 1 (dnum 3): all four modes, count in {1, 2, 16} x batch in {1, 3, 5}"""
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    check(e, orc, ok, 2, 1, MODES, [(c, b) for c in (1, 2, 16) for b in (1, 3, 5)])


@pytest.mark.parametrize("lb,n,nm,K,alpha", [(64, 64, 5, 2, 2), (64, 64, 10, 2, 1), (64, 64, 11, 2, 1), (64, 64, 20, 2, 1), (32, 128, 4, 1, 1),
                                             (16, 4, 2, 1, 1)])
def test_shapes(lb, n, nm, K, alpha, engine_factory, oracle_factory):
    """the shapes of tests/test_gpu_rotate.py: the short last digit; dnum 8 / 9 / 18; 32-bit limbs; rows of 8 bytes, the word
    variants"""
    e, orc, ok = engine_factory(lb, n, nm), oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K)
    check(e, orc, ok, K, alpha, [(False, False), (True, True)], [(1, 3), (2, 5), (16, 1), (2, 3)])


def test_a_row_of_two_chunks(engine_factory, oracle_factory):
    """u64/4096/3: a 32 KiB row is two 16 KiB chunks (k = 2n - 1 takes a tile's source from the other chunk, k = 5 from its own);
    batch 1, count 2.  The hoisted mod-up takes the inverse-transform route here (rows above 2048 words), the sequence the per-digit one"""
    e, orc, ok = engine_factory(64, 4096, 3), oracle_factory(64, 4096, 3), oracle_factory(64, 4096, 2)
    c0, c1, keys, ws, want = setup(e, orc, ok, 1, 1, polys=1)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:2]]
    ks, which = [2 * 4096 - 1, 5], [0, 1]
    for centered, floor in ((False, False), (True, True)):
        w = want(centered, floor, ks, which)
        for plan in PLANS:
            assert same(e, run(e, dc0, dc1, dkeys, dws, ks, which, 1, 1, centered=centered, floor=floor, plan=plan), w), (centered, floor, plan)


def test_c0_null(engine_factory, oracle_factory):
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, ws, want = setup(e, orc, ok, 2, 1)
    dc1, dkeys, dws = e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    for count, unkeyed in ((16, ()), (3, (1,)), (2, (0, 1))):
        ks, which = terms_of(64, count, unkeyed)
        for plan in PLANS:
            assert same(e, run(e, None, dc1, dkeys, dws, ks, which, 2, 1, centered=True, plan=plan), want(True, False, ks, which, with_c0=False)), (count, plan)


def test_unkeyed_terms_take_no_key(engine_factory, oracle_factory):
    """one unkeyed term among keyed ones, and only unkeyed terms: their keys are NULL pointers, so nothing can read them; with no
    keyed term there is no key switch at all (Y = 0) and, without c0, out0 is zero"""
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    check(e, orc, ok, 2, 1, [(False, False), (True, True)], [(4, 3), (16, 5), (2, 1)], unkeyed=(1,))
    check(e, orc, ok, 2, 1, [(False, False)], [(1, 3), (3, 5)], unkeyed=(0, 1, 2))
    c0, c1, keys, ws, want = setup(e, orc, ok, 2, 1)
    for plan in PLANS:
        o0, o1 = run(e, None, e.to_device(c1), [], [e.to_device(w) for w in ws], [1, 1], [None, None], 2, 1, plan=plan)
        assert not bool(o0.any()) and same(e, (o0, o1), want(False, False, [1, 1], [None, None], with_c0=False)), plan
        assert torch.equal(o1, e.automorphism_mac([e.to_device(c1)] * 2, [e.to_device(w) for w in ws[:2]], [1, 1], rows=3))


def test_one_term_k_one_weight_one_is_the_key_switch_plus_c0(engine_factory, oracle_factory):
    """count 1, k = 1, the diagonal of ones: nflhip_keyswitch_ntt_dev word for word, + c0"""
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, ws, want = setup(e, orc, ok, 2, 1)
    dc0, dc1, dkey = e.to_device(c0), e.to_device(c1), e.to_device(keys[1])
    one = torch.ones((5, 64), dtype=torch.int64, device="cuda:0")
    for plan in PLANS:
        for centered, floor in MODES:
            k0, k1 = e.key_switch_ntt(dc1, dkey, 2, 1, centered=centered, floor=floor)
            o0, o1 = e.linear_transform_ntt(None, dc1, [dkey], [one], [1], 2, 1, centered=centered, floor=floor, plan=plan)
            assert torch.equal(o0, k0) and torch.equal(o1, k1), (plan, centered, floor)
            o0, o1 = e.linear_transform_ntt(dc0, dc1, [dkey], [one], [1], 2, 1, centered=centered, floor=floor, plan=plan)
            assert np.array_equal(e.to_host(o0), add_rows(e.to_host(k0), c0, e.P[:3])) and torch.equal(o1, k1), (plan, centered, floor)


def test_adjacent_and_separate_outputs(engine_factory, oracle_factory):
    """out1 right behind out0 (one mod-down of 2 batch polynomials) and apart from it (two)"""
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, ws, want = setup(e, orc, ok, 2, 2)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    ks, which = terms_of(64, 4, (2,))
    w = want(False, False, ks, which)
    for plan in PLANS:
        both = torch.zeros((2,) + c1.shape, dtype=torch.int64, device="cuda:0")
        assert same(e, run(e, dc0, dc1, dkeys, dws, ks, which, 2, 2, out=(both[0], both[1]), plan=plan), w), plan
        far = torch.zeros((3,) + c1.shape, dtype=torch.int64, device="cuda:0")
        assert same(e, run(e, dc0, dc1, dkeys, dws, ks, which, 2, 2, out=(far[2], far[0]), plan=plan), w) and not bool(far[1].any()), plan


def test_batch_one_equals_polynomial_zero_of_batch_three(engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, ws, _ = setup(e, orc, ok, 2, 2)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    ks, which = terms_of(64, 4, (3,))
    for plan in PLANS:
        one = run(e, dc0[:1].contiguous(), dc1[:1].contiguous(), dkeys, dws, ks, which, 2, 2, plan=plan)
        three = run(e, dc0, dc1, dkeys, dws, ks, which, 2, 2, plan=plan)
        assert all(torch.equal(one[c], three[c][:1]) for c in (0, 1)), plan


@pytest.mark.parametrize("with_c0", [True, False])
def test_every_buffer_one_word_off_alignment_with_guard_words(with_c0, engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, ws, want = setup(e, orc, ok, 2, 2)
    ks, which = terms_of(64, 3, (1,))
    w = want(True, False, ks, which, with_c0=with_c0)

    def off(h, fill=0):
        t = torch.full((h.size + 2,), fill, dtype=torch.int64, device="cuda:0")
        t[1:-1].copy_(e.to_device(h).view(-1))
        return t
    a0, a1, ak, aw = off(c0), off(c1), [off(k) for k in keys], [off(x) for x in ws[:3]]
    for plan in PLANS:
        outs = [torch.full((c1.size + 2,), 7, dtype=torch.int64, device="cuda:0") for _ in range(2)]
        e.linear_transform_ntt(a0[1:-1].view(c0.shape) if with_c0 else None, a1[1:-1].view(c1.shape),
                               [None if i is None else ak[i][1:-1] for i in which], [x[1:-1] for x in aw], ks, 2, 2, centered=True,
                               out=(outs[0][1:-1], outs[1][1:-1]), plan=plan)
        for c in (0, 1):
            assert np.array_equal(e.to_host(outs[c][1:-1]).reshape(w[c].shape), w[c]) and int(outs[c][0]) == 7 and int(outs[c][-1]) == 7, plan
    for t, h in [(a0, c0), (a1, c1)] + list(zip(ak + aw, keys + ws[:3])):
        assert int(t[0]) == 0 and int(t[-1]) == 0 and np.array_equal(e.to_host(t[1:-1]).reshape(h.shape), h)


@pytest.mark.parametrize("lb,n,nm,K,alpha", [(64, 64, 5, 2, 2), (32, 128, 4, 1, 1), (16, 4, 2, 1, 1)])
def test_compiled_variant_gives_the_same_words(lb, n, nm, K, alpha, engine_factory, compiled_engine_factory, oracle_factory):
    e, c = engine_factory(lb, n, nm), compiled_engine_factory(lb, n, nm)
    c0, c1, keys, ws, want = setup(e, oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K), K, alpha)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    ks, which = terms_of(n, 3, (2,))
    for centered, floor in ((False, False), (True, True)):
        w = want(centered, floor, ks, which)
        for plan in PLANS:
            assert same(e, run(c, dc0, dc1, dkeys, dws, ks, which, K, alpha, centered=centered, floor=floor, plan=plan), w), (centered, floor, plan)


def test_host_variant_equals_device_variant(engine_factory, oracle_factory):
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, ws, want = setup(e, orc, ok, 2, 2)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    ks, which = terms_of(64, 3, (1,))
    hkeys = [None if i is None else np.array(keys[i]) for i in which]
    for plan in PLANS:
        for centered, floor in ((False, False), (True, True)):
            for with_c0 in (True, False):
                h = e.h_linear_transform_ntt(np.array(c0) if with_c0 else None, np.array(c1), hkeys, [np.array(x) for x in ws[:3]], ks, 2, 2,
                                             centered=centered, floor=floor, plan=plan)
                d = run(e, dc0 if with_c0 else None, dc1, dkeys, dws, ks, which, 2, 2, centered=centered, floor=floor, plan=plan)
                w = want(centered, floor, ks, which, with_c0=with_c0)
                assert all(np.array_equal(h[c], w[c]) for c in (0, 1)), (plan, centered, floor, with_c0)
                assert same(e, d, h)


@pytest.mark.parametrize("plan", ["sequence", "hoisted"])
def test_two_streams_share_the_scratch(plan, engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, ws, want = setup(e, orc, ok, 2, 1)
    b0, b1, keys2, _, want2 = setup(e, orc, ok, 2, 1, seed=11)
    ks, which = terms_of(64, 3, (1,))
    dev = [e.to_device(x) for x in (c0, c1, b0, b1)]
    dk, dk2, dws = [e.to_device(k) for k in keys], [e.to_device(k) for k in keys2], [e.to_device(w) for w in ws]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        r1 = run(e, dev[0], dev[1], dk, dws, ks, which, 2, 1, centered=True, plan=plan, stream=s1)
        r2 = run(e, dev[2], dev[3], dk2, dws, ks, which, 2, 1, centered=True, plan=plan, stream=s2)
    torch.cuda.synchronize()
    assert same(e, r1, want(True, False, ks, which)) and same(e, r2, want2(True, False, ks, which))


@pytest.mark.parametrize("plan", ["sequence", "hoisted"])
def test_graph_capture_replays_identically(plan, engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up call, then the same call captured and replayed three times"""
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, ws, want = setup(e, orc, ok, 2, 2)
    ks, which = terms_of(64, 3, (1,))
    w = want(True, False, ks, which)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(x) for x in ws]
    both = torch.zeros((2,) + c1.shape, dtype=torch.int64, device="cuda:0")
    out = (both[0], both[1])

    def go():
        run(e, dc0, dc1, dkeys, dws, ks, which, 2, 2, centered=True, out=out, plan=plan)

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        go()                                                   # the warm-up: tables, scratch and child contexts of this batch
        st.synchronize()
        assert same(e, out, w)
        with torch.cuda.graph(g, stream=st):
            go()
    for _ in range(3):
        both.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(e, out, w)


def test_first_call_while_capturing_is_refused_and_the_stream_stays_usable(oracle_factory):
    import torch
    from nfllib_amd import Engine, _lib
    e, orc, ok = Engine(64, 64, 5, device=0), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)   # a context of its own: nothing is warm
    try:
        c0, c1, keys, ws, want = setup(e, orc, ok, 2, 2)
        ks, which = terms_of(64, 2)
        w = want(False, False, ks, which)
        dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(x) for x in ws[:2]]
        f = _lib.lib.nflhip_lintrans_ntt_dev
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        z = torch.zeros(4, device="cuda:0")
        pk, pw, kv = (C.c_void_p * 2)(*[dkeys[i].data_ptr() for i in which]), (C.c_void_p * 2)(*[x.data_ptr() for x in dws]), (C.c_uint64 * 2)(*ks)
        torch.cuda.synchronize()
        for flags in (_lib.LINTRANS_HOISTED, _lib.LINTRANS_SEQUENCE):   # (each plan is cold in its turn)
            o = torch.full((2,) + c1.shape, 5, dtype=torch.int64, device="cuda:0")
            args = (e.ctx, o[0].data_ptr(), o[1].data_ptr(), dc0.data_ptr(), dc1.data_ptr(), pk, pw, kv, 2, 3, 2, 2, flags, sp)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    z.add_(1)
                    rc = f(*args)
            torch.cuda.synchronize()
            assert rc == _lib.ERR_UNSUPPORTED, (flags, rc)
            assert bool((o == 5).all())                                  # nothing was enqueued
            assert f(*args) == 0                                         # the same stream
            st.synchronize()
            assert same(e, (o[0], o[1]), w), flags
    finally:
        e.close()


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    from nfllib_amd.params import params
    Lb, ERR = _lib.lib, _lib.ERR_INVALID
    N, nm, K, alpha = 64, 5, 2, 2
    e = engine_factory(64, N, nm)
    row, batch, L, dnum, count = N * 8, 2, nm - K, 2, 2
    c = torch.ones((2, batch, L, N), dtype=torch.int64, device="cuda:0")
    k = torch.ones((2, dnum, 2, nm, N), dtype=torch.int64, device="cuda:0")
    w = torch.ones((2, nm, N), dtype=torch.int64, device="cuda:0")
    o = torch.full((2, batch, L, N), 9, dtype=torch.int64, device="cuda:0")
    pc0, pc1, pk, pw = c[0].data_ptr(), c[1].data_ptr(), [k[0].data_ptr(), k[1].data_ptr()], [w[0].data_ptr(), w[1].data_ptr()]
    po0, po1 = o[0].data_ptr(), o[1].data_ptr()
    f, hf = Lb.nflhip_lintrans_ntt_dev, Lb.nflhip_lintrans_ntt

    def arr(xs, n=17):
        return None if xs is None else (C.c_void_p * n)(*xs)

    def call(ctx=e.ctx, o0=po0, o1=po1, c0=pc0, c1=pc1, keys=pk, ws=pw, ks=(5, 25), cnt=count, b=batch, kk=K, al=alpha, flags=0, fn=f):
        kv = None if ks is None else (C.c_uint64 * 17)(*ks)
        tail = (None,) if fn is f else ()
        return fn(ctx, o0, o1, c0, c1, arr(keys), arr(ws), kv, cnt, b, kk, al, flags, *tail)

    assert call(ctx=None) == ERR                                                          # NULL context
    for kw in (dict(o0=None), dict(o1=None), dict(c1=None), dict(keys=None), dict(ws=None), dict(ks=None)):
        assert call(**kw) == ERR, kw                                                      # a NULL pointer (c0 alone may be NULL)
    assert call(keys=[pk[0], None]) == ERR and call(keys=[None, pk[1]], ks=(2 * N + 5, 25)) == ERR    # a NULL key with k != 1 mod 2n
    assert call(ws=[pw[0], None]) == ERR and call(ws=[None, pw[1]], keys=[None, pk[1]], ks=(1, 5)) == ERR   # a NULL weight
    assert call(cnt=0) == ERR and call(cnt=17, keys=(pk * 9)[:17], ws=(pw * 9)[:17], ks=(5,) * 17) == ERR   # count out of range
    for ks in ((4, 5), (5, 0), (5, 2**64 - 2)):
        assert call(ks=ks) == ERR, ks                                                     # an even k
    for kk in (0, nm, nm + 1, 2**64 - 1):
        assert call(kk=kk, al=1) == ERR, kk                                               # k_special out of range
    for al in (0, L + 1, 2**64 - 1):
        assert call(al=al) == ERR, al                                                     # alpha out of range
    for flags in (1, 2, 0x80, 0x400, 0x800, 0x4000, -1, 0x3000, 0x3100):                  # unknown bits; two plan flags
        assert call(flags=flags) == ERR, flags
    assert call(b=2**61) == ERR                                                           # the size overflows
    ob, kb, wb = batch * L * row, 2 * dnum * nm * row, nm * row
    for kw in (dict(o1=po0), dict(o1=po0 + ob - 8), dict(o0=pc0), dict(o1=pc0 + ob - 8), dict(o0=pc1 - ob + 8), dict(o1=pc1),
               dict(o0=pk[1]), dict(o1=pk[0] + kb - 8), dict(o0=pk[1] - ob + 8),
               dict(o0=pw[0]), dict(o1=pw[1] + wb - 8), dict(o0=pw[1] - ob + 8)):         # the outputs; with c0, c1; a key; a weight
        assert call(**kw) == ERR, kw
    h = [np.ones((batch, L, N), np.uint64) for _ in range(4)]
    hk = [np.ones((dnum, 2, nm, N), np.uint64) for _ in range(2)]
    hw = [np.ones((nm, N), np.uint64) for _ in range(2)]
    host = dict(fn=hf, o0=h[0].ctypes.data, o1=h[1].ctypes.data, c0=h[2].ctypes.data, c1=h[3].ctypes.data, keys=[x.ctypes.data for x in hk],
                ws=[x.ctypes.data for x in hw])
    assert call(**dict(host, o1=h[0].ctypes.data)) == ERR                                 # host: overlap
    assert call(**dict(host, c1=None)) == ERR and call(**dict(host, al=0)) == ERR and call(**dict(host, flags=0x3000)) == ERR
    assert call(**dict(host, ks=(5, 6))) == ERR and call(**dict(host, cnt=0)) == ERR and call(**dict(host, keys=[None, hk[1].ctypes.data])) == ERR
    for flags in (0, 0x1000, 0x2000):
        assert call(o0=None, o1=None, c0=None, c1=None, keys=None, ws=None, ks=None, b=0, flags=flags) == 0     # an empty batch is fine
    assert call(fn=hf, o0=None, o1=None, c0=None, c1=None, keys=None, ws=None, ks=None, b=0) == 0
    # a repeated modulus inside a digit, or among the special rows, is refused by the table builder, on the host
    pr = params(64)
    for idx, kk, al in (([0, 0, 1, 2], 1, 2), ([0, 1, 2, 2], 2, 1)):
        tabs = [np.ascontiguousarray(t[idx]) for t in (pr.P, pr.primitive_roots, pr.invkmax)]
        ctx = C.c_void_p()
        assert Lb.nflhip_ctx_create(C.byref(ctx), 0, 64, N, 4, *[t.ctypes.data_as(C.c_void_p) for t in tabs], pr.kmax_log2) == 0
        try:
            for flags in (0, 0x1000, 0x2000):
                assert call(ctx=ctx, b=1, kk=kk, al=al, flags=flags) == ERR, (idx, flags)
                assert b"baseconv: a source modulus repeats" in Lb.nflhip_last_error(ctx)        # the builder's own message
        finally:
            torch.cuda.synchronize()
            Lb.nflhip_ctx_destroy(ctx)
    # nothing refused above wrote anything, and the context still works
    torch.cuda.synchronize()
    assert bool((o == 9).all()) and bool((k == 1).all()) and bool((c == 1).all()) and bool((w == 1).all())
    assert call(keys=[pk[0], pk[0]], ws=[pw[0], pw[0]], ks=(1, 1), c0=None) == 0         # keys, weights and ks may repeat; a keyed k = 1
    torch.cuda.synchronize()
    assert bool((o != 9).all())
    first = o[0].clone()
    assert call(c0=None, keys=[pk[0], pk[0]], ws=[pw[0], pw[0]], ks=(1, 1), o0=pc0) == 0   # (without c0 its memory is free to use)
    torch.cuda.synchronize()
    assert torch.equal(c[0], first)


@pytest.fixture(scope="module")
def cpp_program(tmp_path_factory):
    from test_lintrans_cpp import build_cpp
    return build_cpp(str(tmp_path_factory.mktemp("cpp_lintrans")), gpu=True)


@pytest.mark.parametrize("batch", [1, 5])
def test_cpp_surface_on_the_gpu(cpp_program, batch):
    """the program of tests/cpp_lintrans against the real library: poly, poly_p and device_batch equal to each other and to the sums
    written by hand, and the keys and diagonals used through device_batches equal to those used through raw pointers"""
    import os
    import subprocess
    r = subprocess.run([cpp_program, str(batch)], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
