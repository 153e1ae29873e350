"""GPU: hoisted rotations (include/nflhip.h "hoisted rotations"; nfllib_amd/csrc/kernels_rotate.hip, kernels_dot_multi.hip and the plans
of api.hip).  Both plans and the default, both mod-up modes and both roundings, word for word against tests/rotate_util.py
rotate_rns: the header's definition on Python integers between the CPU oracle's transforms.  No tolerance anywhere.  c1 is planted
as tests/test_gpu_keyswitch.py plants its input (per digit the edge values, the centred band, every y_i = p_i - 1); the keys are
random.  The restatement works polynomial by polynomial, so it is computed once per shape and mode on the planted batch of three
and indexed for the other batch sizes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from keyswitch_util import digits
from rotate_util import rotate_rns
from test_gpu_keyswitch import planted

pytestmark = pytest.mark.gpu

PLANS = ("sequence", "hoisted", None)
MODES = [(c, f) for c in (False, True) for f in (False, True)]
PICK = {1: [0], 3: [0, 1, 2], 5: [0, 1, 2, 0, 1]}      # the planted polynomials a batch of 1 / 3 / 5 is made of
_CACHE = {}


def rotations(n, count):
    """(k, index of the key) per rotation: k = 1, 2n - 1, 5, 25, then 5 AGAIN with the other key, then further odd k"""
    ks = [1, 2 * n - 1, 5, 25, 5] + [(2 * i + 3) % (2 * n) for i in range(count)]
    key = [0, 1, 0, 1, 1] + [i % 2 for i in range(count)]
    return (ks[:count], key[:count]) if count > 1 else ([5], [0])


def case(e, orc, ok, K, alpha, seed=3, polys=3):
    """c0, c1 (NTT form, [polys, L, n]), two keys and, computed on demand and kept, per mode the two key switches + c0 of the
    restatement, from which every rotation's expected words are a permutation"""
    key = (e.limb_bits, e.degree, e.nmoduli, K, alpha, seed, polys)
    if key not in _CACHE:
        nm, n, L = e.nmoduli, e.degree, e.nmoduli - K
        dnum = len(digits(nm, K, alpha))
        c1 = ok.ntt(planted(e, K, alpha, seed)[:polys])
        c0 = B.random_batch(e.P[:L], n, polys, e.np_dtype, seed + 50)
        c0[0, :, :2] = np.array([int(p) - 1 for p in e.P[:L]], dtype=e.np_dtype)[:, None]      # the sum's wrap: p - 1 + anything
        c0[-1, :, -1] = 0
        keys = [B.random_batch(e.P, n, 2 * dnum, e.np_dtype, seed + 100 + i).reshape(dnum, 2, nm, n) for i in range(2)]
        for x in [c0, c1] + keys:
            x.setflags(write=False)
        _CACHE[key] = (c0, c1, keys, {})
    c0, c1, keys, memo = _CACHE[key]

    def want(centered, floor, ks, which, with_c0=True, pick=None):
        m = memo.setdefault((centered, floor), {})
        r = rotate_rns(c0 if with_c0 else None, c1, [keys[i] for i in which], ks, e.P, K, alpha, centered, floor, orc, ok, memo=m)
        return r if pick is None else [(a[pick], b[pick]) for a, b in r]
    return c0, c1, keys, want


def run(e, dc0, dc1, dkeys, ks, which, K, alpha, **kw):
    return e.rotate_hoisted_ntt(dc0, dc1, [dkeys[i] for i in which], ks, K, alpha, **kw)


def same(e, got, want):
    return len(got) == len(want) and all(np.array_equal(e.to_host(g[c]), w[c]) for g, w in zip(got, want) for c in (0, 1))


def check(e, orc, ok, K, alpha, modes, combos, plans=PLANS):
    c0, c1, keys, want = case(e, orc, ok, K, alpha)
    dkeys = [e.to_device(k) for k in keys]
    for count, batch in combos:
        ks, which = rotations(e.degree, count)
        pick = PICK[batch]
        dc0, dc1 = e.to_device(c0[pick]), e.to_device(c1[pick])
        for centered, floor in modes:
            w = want(centered, floor, ks, which, pick=pick)
            for plan in plans:
                got = run(e, dc0, dc1, dkeys, ks, which, K, alpha, centered=centered, floor=floor, plan=plan)
                assert got[0][0].shape == dc1.shape
                assert same(e, got, w), (K, alpha, count, batch, centered, floor, plan)
        assert np.array_equal(e.to_host(dc0), c0[pick]) and np.array_equal(e.to_host(dc1), c1[pick])     # the inputs are unchanged
    assert all(np.array_equal(e.to_host(d), k) for d, k in zip(dkeys, keys))


def test_every_plan_every_mode_every_count_and_batch(engine_factory, oracle_factory):
    """u64/64/5, K 2, alpha 1 (dnum 3): all four modes, count in {1, 2, 16} x batch in {1, 3, 5}"""
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    check(e, orc, ok, 2, 1, MODES, [(c, b) for c in (1, 2, 16) for b in (1, 3, 5)])


@pytest.mark.parametrize("lb,n,nm,K,alpha", [(64, 64, 5, 2, 2), (64, 64, 10, 2, 1), (64, 64, 11, 2, 1), (64, 64, 20, 2, 1), (32, 128, 4, 1, 1),
                                             (16, 4, 2, 1, 1)])
def test_shapes(lb, n, nm, K, alpha, engine_factory, oracle_factory):
    """the short last digit; dnum 8, the register form's last size; dnum 9, the streaming form's first; dnum 18, across the 16-term
    chunk; 32-bit limbs; rows of 8 bytes, the word variants (u16/4/2 is the one 16-bit parameter set there is)"""
    e, orc, ok = engine_factory(lb, n, nm), oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K)
    check(e, orc, ok, K, alpha, [(False, False), (True, True)], [(1, 3), (2, 5), (16, 1), (2, 3)])


def test_a_row_of_two_chunks(engine_factory, oracle_factory):
    """u64/4096/3: a 32 KiB row is two 16 KiB chunks, the permutation's chunk-to-chunk path (k = 2n - 1 sends a chunk to the other
    one, k = 5 keeps it); batch 1, count 2.  The mod-up takes the inverse-transform route here (rows above 2048 words)"""
    e, orc, ok = engine_factory(64, 4096, 3), oracle_factory(64, 4096, 3), oracle_factory(64, 4096, 2)
    c0, c1, keys, want = case(e, orc, ok, 1, 1, polys=1)
    dc0, dc1, dkeys = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys]
    ks, which = [2 * 4096 - 1, 5], [0, 1]
    for centered, floor in ((False, False), (True, True)):
        w = want(centered, floor, ks, which)
        for plan in PLANS:
            assert same(e, run(e, dc0, dc1, dkeys, ks, which, 1, 1, centered=centered, floor=floor, plan=plan), w), (centered, floor, plan)


def test_c0_null_and_the_plain_key_switch(engine_factory, oracle_factory):
    """without c0 the sums are the key switch's; count = 1, k = 1 is nflhip_keyswitch_ntt_dev word for word"""
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, want = case(e, orc, ok, 2, 1)
    dc1, dkeys = e.to_device(c1), [e.to_device(k) for k in keys]
    ks, which = rotations(64, 16)
    for plan in PLANS:
        assert same(e, run(e, None, dc1, dkeys, ks, which, 2, 1, centered=True, plan=plan), want(True, False, ks, which, with_c0=False)), plan
        for centered, floor in MODES:
            (o0, o1), = run(e, None, dc1, dkeys, [1], [1], 2, 1, centered=centered, floor=floor, plan=plan)
            k0, k1 = e.key_switch_ntt(dc1, dkeys[1], 2, 1, centered=centered, floor=floor)
            assert torch.equal(o0, k0) and torch.equal(o1, k1), (plan, centered, floor)


def test_batch_one_equals_polynomial_zero_of_batch_three(engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, _ = case(e, orc, ok, 2, 2)
    dc0, dc1, dkeys = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys]
    ks, which = rotations(64, 4)
    for plan in PLANS:
        one = run(e, dc0[:1].contiguous(), dc1[:1].contiguous(), dkeys, ks, which, 2, 2, plan=plan)
        three = run(e, dc0, dc1, dkeys, ks, which, 2, 2, plan=plan)
        assert all(torch.equal(a[c], b[c][:1]) for a, b in zip(one, three) for c in (0, 1)), plan


@pytest.mark.parametrize("with_c0", [True, False])
def test_every_buffer_one_word_off_alignment_with_guard_words(with_c0, engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, want = case(e, orc, ok, 2, 2)
    ks, which = rotations(64, 3)
    w = want(True, False, ks, which, with_c0=with_c0)

    def off(h, fill=0):
        t = torch.full((h.size + 2,), fill, dtype=torch.int64, device="cuda:0")
        t[1:-1].copy_(e.to_device(h).view(-1))
        return t
    a0, a1, ak = off(c0), off(c1), [off(k) for k in keys]
    for plan in PLANS:
        outs = [tuple(torch.full((c1.size + 2,), 7, dtype=torch.int64, device="cuda:0") for _ in range(2)) for _ in ks]
        e.rotate_hoisted_ntt(a0[1:-1].view(c0.shape) if with_c0 else None, a1[1:-1].view(c1.shape), [ak[i][1:-1] for i in which], ks, 2, 2,
                             centered=True, outs=[(o[0][1:-1], o[1][1:-1]) for o in outs], plan=plan)
        for o, x in zip(outs, w):
            for c in (0, 1):
                assert np.array_equal(e.to_host(o[c][1:-1]).reshape(x[c].shape), x[c]) and int(o[c][0]) == 7 and int(o[c][-1]) == 7, plan
    for t, h in [(a0, c0), (a1, c1)] + list(zip(ak, keys)):
        assert int(t[0]) == 0 and int(t[-1]) == 0 and np.array_equal(e.to_host(t[1:-1]).reshape(h.shape), h)


@pytest.mark.parametrize("lb,n,nm,K,alpha", [(64, 64, 5, 2, 2), (32, 128, 4, 1, 1), (16, 4, 2, 1, 1)])
def test_compiled_variant_gives_the_same_words(lb, n, nm, K, alpha, engine_factory, compiled_engine_factory, oracle_factory):
    e, c = engine_factory(lb, n, nm), compiled_engine_factory(lb, n, nm)
    c0, c1, keys, want = case(e, oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K), K, alpha)
    dc0, dc1, dkeys = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys]
    ks, which = rotations(n, 3)
    for centered, floor in ((False, False), (True, True)):
        w = want(centered, floor, ks, which)
        for plan in PLANS:
            assert same(e, run(c, dc0, dc1, dkeys, ks, which, K, alpha, centered=centered, floor=floor, plan=plan), w), (centered, floor, plan)


def test_host_variant_equals_device_variant(engine_factory, oracle_factory):
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, want = case(e, orc, ok, 2, 2)
    dc0, dc1, dkeys = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys]
    ks, which = rotations(64, 3)
    for plan in PLANS:
        for centered, floor in ((False, False), (True, True)):
            for with_c0 in (True, False):
                h = e.h_rotate_hoisted_ntt(np.array(c0) if with_c0 else None, np.array(c1), [np.array(keys[i]) for i in which], ks, 2, 2,
                                           centered=centered, floor=floor, plan=plan)
                d = run(e, dc0 if with_c0 else None, dc1, dkeys, ks, which, 2, 2, centered=centered, floor=floor, plan=plan)
                w = want(centered, floor, ks, which, with_c0=with_c0)
                assert all(np.array_equal(h[m][c], w[m][c]) for m in range(3) for c in (0, 1)), (plan, centered, floor, with_c0)
                assert same(e, d, h)


@pytest.mark.parametrize("plan", ["sequence", "hoisted"])
def test_two_streams_share_the_scratch(plan, engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, want = case(e, orc, ok, 2, 1)
    b0, b1, keys2, want2 = case(e, orc, ok, 2, 1, seed=11)
    ks, which = rotations(64, 3)
    dev = [e.to_device(x) for x in (c0, c1, b0, b1)]
    dk, dk2 = [e.to_device(k) for k in keys], [e.to_device(k) for k in keys2]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        r1 = run(e, dev[0], dev[1], dk, ks, which, 2, 1, centered=True, plan=plan, stream=s1)
        r2 = run(e, dev[2], dev[3], dk2, ks, which, 2, 1, centered=True, plan=plan, stream=s2)
    torch.cuda.synchronize()
    assert same(e, r1, want(True, False, ks, which)) and same(e, r2, want2(True, False, ks, which))


@pytest.mark.parametrize("plan", ["sequence", "hoisted"])
def test_graph_capture_replays_identically(plan, engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up call, then the same call captured and replayed three times"""
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    c0, c1, keys, want = case(e, orc, ok, 2, 2)
    ks, which = rotations(64, 3)
    w = want(True, False, ks, which)
    dc0, dc1, dkeys = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys]
    both = torch.zeros((3, 2) + c1.shape, dtype=torch.int64, device="cuda:0")
    outs = [(both[m, 0], both[m, 1]) for m in range(3)]

    def go():
        run(e, dc0, dc1, dkeys, ks, which, 2, 2, centered=True, outs=outs, plan=plan)

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        go()                                                   # the warm-up: tables, scratch and child contexts of this batch
        st.synchronize()
        assert same(e, outs, w)
        with torch.cuda.graph(g, stream=st):
            go()
    for _ in range(3):
        both.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(e, outs, w)


def test_first_call_while_capturing_is_refused_and_the_stream_stays_usable(oracle_factory):
    import torch
    from nfllib_amd import Engine, _lib
    e, orc, ok = Engine(64, 64, 5, device=0), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)   # a context of its own: nothing is warm
    try:
        c0, c1, keys, want = case(e, orc, ok, 2, 2)
        ks, which = rotations(64, 2)
        w = want(False, False, ks, which)
        dc0, dc1, dkeys = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys]
        f = _lib.lib.nflhip_rotate_hoisted_ntt_dev
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        z = torch.zeros(4, device="cuda:0")
        pk, kv = (C.c_void_p * 2)(*[dkeys[i].data_ptr() for i in which]), (C.c_uint64 * 2)(*ks)
        torch.cuda.synchronize()
        for flags in (_lib.ROTATE_HOISTED, _lib.ROTATE_SEQUENCE):   # (each plan is cold in its turn)
            o = torch.full((2, 2) + c1.shape, 5, dtype=torch.int64, device="cuda:0")
            p0, p1 = (C.c_void_p * 2)(o[0, 0].data_ptr(), o[1, 0].data_ptr()), (C.c_void_p * 2)(o[0, 1].data_ptr(), o[1, 1].data_ptr())
            args = (e.ctx, p0, p1, dc0.data_ptr(), dc1.data_ptr(), pk, kv, 2, 3, 2, 2, flags, sp)
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
            assert same(e, [(o[m, 0], o[m, 1]) for m in range(2)], w), flags
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
    o = torch.full((count, 2, batch, L, N), 9, dtype=torch.int64, device="cuda:0")
    pc0, pc1, pk = c[0].data_ptr(), c[1].data_ptr(), [k[0].data_ptr(), k[1].data_ptr()]
    po0, po1 = [o[m, 0].data_ptr() for m in range(count)], [o[m, 1].data_ptr() for m in range(count)]
    f, hf = Lb.nflhip_rotate_hoisted_ntt_dev, Lb.nflhip_rotate_hoisted_ntt

    def arr(xs, n=17):
        return None if xs is None else (C.c_void_p * n)(*xs)

    def call(ctx=e.ctx, o0=po0, o1=po1, c0=pc0, c1=pc1, keys=pk, ks=(5, 25), cnt=count, b=batch, kk=K, al=alpha, flags=0, fn=f):
        kv = None if ks is None else (C.c_uint64 * 17)(*ks)
        tail = (None,) if fn is f else ()
        return fn(ctx, arr(o0), arr(o1), c0, c1, arr(keys), kv, cnt, b, kk, al, flags, *tail)

    assert call(ctx=None) == ERR                                                          # NULL context
    for kw in (dict(o0=None), dict(o1=None), dict(c1=None), dict(keys=None), dict(ks=None), dict(o0=[po0[0], None]), dict(o1=[None, po1[1]]),
               dict(keys=[pk[0], None])):
        assert call(**kw) == ERR, kw                                                      # a NULL pointer (c0 alone may be NULL)
    assert call(cnt=0) == ERR and call(cnt=17, o0=(po0 * 9)[:17], o1=(po1 * 9)[:17], keys=(pk * 9)[:17], ks=(5,) * 17) == ERR   # count out of range
    for ks in ((4, 5), (5, 0), (5, 2**64 - 2)):
        assert call(ks=ks) == ERR, ks                                                     # an even k
    for kk in (0, nm, nm + 1, 2**64 - 1):
        assert call(kk=kk, al=1) == ERR, kk                                               # k_special out of range
    for al in (0, L + 1, 2**64 - 1):
        assert call(al=al) == ERR, al                                                     # alpha out of range
    for flags in (1, 2, 0x80, 0x400, 0x800, 0x4000, -1, 0x3000, 0x3100):                  # unknown bits; two plan flags
        assert call(flags=flags) == ERR, flags
    assert call(b=2**61) == ERR                                                           # the size overflows
    ob, kb = batch * L * row, 2 * dnum * nm * row
    for kw in (dict(o0=[po0[0], po0[0]]), dict(o1=[po1[0], po0[0] + ob - 8]), dict(o0=[po0[0], po1[1]]),           # among the outputs
               dict(o0=[pc0, po0[1]]), dict(o1=[po1[0], pc0 + ob - 8]), dict(o0=[pc1 - ob + 8, po0[1]]), dict(o1=[pc1, po1[1]]),   # with c0, c1
               dict(o0=[pk[1], po0[1]]), dict(o1=[po1[0], pk[0] + kb - 8]), dict(o0=[po0[0], pk[1] - ob + 8])):    # with a key, of another rotation too
        assert call(**kw) == ERR, kw
    h = [np.ones((batch, L, N), np.uint64) for _ in range(6)]
    hk = [np.ones((dnum, 2, nm, N), np.uint64) for _ in range(2)]
    hp = [x.ctypes.data for x in h]
    host = dict(fn=hf, o0=hp[:2], o1=hp[2:4], c0=hp[4], c1=hp[5], keys=[x.ctypes.data for x in hk])
    assert call(**dict(host, o1=[hp[2], hp[0]])) == ERR                                   # host: overlap
    assert call(**dict(host, c1=None)) == ERR and call(**dict(host, al=0)) == ERR and call(**dict(host, flags=0x3000)) == ERR
    assert call(**dict(host, ks=(5, 6))) == ERR and call(**dict(host, cnt=0)) == ERR
    for flags in (0, 0x1000, 0x2000):
        assert call(o0=None, o1=None, c0=None, c1=None, keys=None, ks=None, b=0, flags=flags) == 0     # an empty batch is fine
    assert call(fn=hf, o0=None, o1=None, c0=None, c1=None, keys=None, ks=None, b=0) == 0
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
            assert call(ctx=ctx, o0=None, o1=None, c0=None, c1=None, keys=None, ks=None, b=0, kk=kk, al=al) == 0
        finally:
            torch.cuda.synchronize()
            Lb.nflhip_ctx_destroy(ctx)
    # nothing refused above wrote anything, and the context still works
    torch.cuda.synchronize()
    assert bool((o == 9).all()) and bool((k == 1).all()) and bool((c == 1).all())
    assert call(keys=[pk[0], pk[0]], ks=(1, 1), c0=None) == 0                             # keys may repeat, a k may repeat, k = 1 is allowed
    torch.cuda.synchronize()
    assert bool((o != 9).all())
    first = o[0, 0].clone()
    assert call(c0=None, o0=[pc0, po0[1]]) == 0                                           # (without c0 its memory is free to use)
    torch.cuda.synchronize()
    assert torch.equal(c[0], first)


@pytest.fixture(scope="module")
def cpp_program(tmp_path_factory):
    from test_rotate_cpu import build_cpp
    return build_cpp(str(tmp_path_factory.mktemp("cpp_rotate")), gpu=True)


@pytest.mark.parametrize("batch", [1, 5])
def test_cpp_surface_on_the_gpu(cpp_program, batch):
    """the program of tests/cpp_rotate against the real library: poly, poly_p and device_batch equal to the definition written by hand
    through the existing header calls, and the keys used through device_batches equal to the keys used through raw pointers"""
    r = subprocess.run([cpp_program, str(batch)], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
