"""GPU: the weighted sum of NTT-form automorphisms (include/nflhip.h "weighted sums of automorphisms";
nfllib_amd/csrc/kernels_lintrans.hip k_permute_mac_ntt), word for word against tests/lintrans_util.py mac_rns -- the header's formula on
Python integers.  No tolerance anywhere.  Both staging variants (one buffer, two) are checked everywhere: same words."""
import ctypes as C

import numpy as np
import pytest

import baseconv_util as B
from lintrans_util import mac_rns

pytestmark = pytest.mark.gpu


def multipliers(n, terms):
    """k = 1, 2n - 1 (moves a chunk to another), 5 (keeps it), 25, then further odd k"""
    return ([1, 2 * n - 1, 5, 25] + [(2 * i + 3) % (2 * n) for i in range(terms)])[:terms]


def operands(e, rows, terms, batch, seed=1):
    """terms inputs [batch, rows, n] and weights [nm, n], canonical and random, with the edge words 0 and p - 1 planted"""
    n, P = e.degree, e.P
    ins = [B.random_batch(P[:rows], n, batch, e.np_dtype, seed + t) for t in range(terms)]
    ws = [B.random_batch(P, n, 1, e.np_dtype, seed + 100 + t)[0] for t in range(terms)]
    pm1 = np.array([int(p) - 1 for p in P], dtype=e.np_dtype)
    ins[0][0, :, :2] = pm1[:rows, None]
    ws[0][:, :3] = pm1[:, None]
    ins[-1][-1, :, -1] = 0
    ws[-1][:, -1] = 0
    return ins, ws


def check(e, rows, terms, batch, seed=1, modes=("none", "separate", "in place")):
    ins, ws = operands(e, rows, terms, batch, seed)
    ks = multipliers(e.degree, terms)
    add = B.random_batch(e.P[:rows], e.degree, batch, e.np_dtype, seed + 999)
    add[0, :, 0] = np.array([int(p) - 1 for p in e.P[:rows]], dtype=e.np_dtype)              # the final sum's wrap
    want = {"none": mac_rns(ins, ws, ks, e.P[:rows])}
    want["separate"] = want["in place"] = mac_rns(ins, ws, ks, e.P[:rows], addend=add)
    di, dw, da = [e.to_device(x) for x in ins], [e.to_device(w) for w in ws], e.to_device(add)
    for double in (False, True):
        for mode in modes:
            if mode == "in place":
                out = da.clone()
                got = e.automorphism_mac(di, dw, ks, addend=out, out=out, rows=rows, double_buffer=double)
            else:
                got = e.automorphism_mac(di, dw, ks, addend=da if mode == "separate" else None, rows=rows, double_buffer=double)
            assert np.array_equal(e.to_host(got), want[mode]), (rows, terms, batch, mode, double)
    assert all(np.array_equal(e.to_host(d), h) for d, h in zip(di + dw + [da], ins + ws + [add]))   # the inputs are unchanged


@pytest.mark.parametrize("rows", [5, 3])
def test_every_term_count_and_batch_on_leading_rows(rows, engine_factory):
    """u64/64/5: rows = nm and rows = 3 of 5 (the weights keep their nm-row stride); terms in {1, 2, 16} x batch in {1, 3, 5};
    several whole rows per tile, the last tile short"""
    e = engine_factory(64, 64, 5)
    for terms in (1, 2, 16):
        for batch in (1, 3, 5):
            check(e, rows, terms, batch)


@pytest.mark.parametrize("lb,n,nm,combos", [
    (32, 128, 4, [(1, 3), (2, 5), (16, 1)]),          # 32-bit limbs
    (16, 4, 2, [(1, 1), (2, 3), (16, 5)]),            # rows of 8 bytes: the word variant
    (64, 4096, 3, [(2, 1), (16, 3)]),                 # two chunks per row: k = 2n - 1 moves a chunk, k = 5 keeps it
    (64, 8192, 2, [(2, 1), (4, 3)]),                  # four chunks per row
])
def test_shapes(lb, n, nm, combos, engine_factory):
    e = engine_factory(lb, n, nm)
    for terms, batch in combos:
        check(e, nm, terms, batch, modes=("none", "in place"))


@pytest.mark.parametrize("lb,n,nm", [(64, 64, 96), (32, 128, 4), (16, 4, 2)])
def test_the_accumulators_edge(lb, n, nm, engine_factory):
    """16 terms with every input word and every weight word p_j - 1: the largest sum the unreduced accumulator has to hold
    (16 (p - 1)^2 < 2^(2W)); u64/64/96 reaches the moduli with the largest delta (2^62 - p >= 2^32 from the 93rd on)"""
    e = engine_factory(lb, n, nm)
    batch = 2
    pm1 = np.array([int(p) - 1 for p in e.P], dtype=e.np_dtype)
    x = np.ascontiguousarray(np.broadcast_to(pm1[None, :, None], (batch, nm, n)))
    w = np.ascontiguousarray(np.broadcast_to(pm1[:, None], (nm, n)))
    dx, dw = e.to_device(x), e.to_device(w)
    ks = multipliers(n, 16)
    want = np.empty_like(x)
    for j, p in enumerate(e.P):
        want[:, j] = (16 * (int(p) - 1) ** 2 + int(p) - 1) % int(p)
    for double in (False, True):
        got = e.automorphism_mac([dx] * 16, [dw] * 16, ks, addend=dx, double_buffer=double)
        assert np.array_equal(e.to_host(got), want), double
    assert np.array_equal(want, mac_rns([x] * 16, [w] * 16, ks, e.P, addend=x))


def test_a_repeated_input_and_k_one(engine_factory):
    """ins may repeat; k = 1 with weight 1 and no other term copies the input; two terms of one input with weights w and p - w cancel"""
    import torch
    e = engine_factory(64, 64, 5)
    (x,), (w,) = operands(e, 5, 1, 3)
    dx, dw = e.to_device(x), e.to_device(w)
    one = torch.ones((5, 64), dtype=torch.int64, device="cuda:0")
    assert torch.equal(e.automorphism_mac([dx], [one], [1]), dx)
    neg = np.empty_like(w)
    for j, p in enumerate(e.P):
        neg[j] = (int(p) - w[j].astype(object)) % int(p)
    got = e.automorphism_mac([dx, dx, dx], [dw, e.to_device(neg), dw], [5, 5, 2 * 64 - 1])
    assert np.array_equal(e.to_host(got), mac_rns([x], [w], [2 * 64 - 1], e.P))


@pytest.mark.parametrize("lb,n,nm", [(64, 64, 5), (64, 4096, 3), (32, 128, 4)])
def test_every_buffer_one_word_off_alignment_with_guard_words(lb, n, nm, engine_factory):
    """the word variant on rows that the 16-byte variant serves otherwise; nothing is written outside the output"""
    import torch
    e = engine_factory(lb, n, nm)
    terms, batch = 3, 2
    ins, ws = operands(e, nm, terms, batch, seed=7)
    add = B.random_batch(e.P, n, batch, e.np_dtype, 77)
    ks = multipliers(n, terms)
    want = mac_rns(ins, ws, ks, e.P, addend=add)

    def off(h, fill=0):
        t = torch.full((h.size + 2,), fill, dtype=e.torch_dtype, device="cuda:0")
        t[1:-1].copy_(e.to_device(h).view(-1))
        return t
    gi, gw, ga = [off(x) for x in ins], [off(w) for w in ws], off(add)
    for double in (False, True):
        out = torch.full((add.size + 2,), 7, dtype=e.torch_dtype, device="cuda:0")
        e.automorphism_mac([t[1:-1] for t in gi], [t[1:-1] for t in gw], ks, addend=ga[1:-1], out=out[1:-1], double_buffer=double)
        assert np.array_equal(e.to_host(out[1:-1]).reshape(want.shape), want) and int(out[0]) == 7 and int(out[-1]) == 7, double
    for t, h in zip(gi + gw + [ga], ins + ws + [add]):
        assert int(t[0]) == 0 and int(t[-1]) == 0 and np.array_equal(e.to_host(t[1:-1]).reshape(h.shape), h)


def test_host_variant_equals_device_variant(engine_factory):
    e = engine_factory(64, 64, 5)
    for rows in (5, 3):
        ins, ws = operands(e, rows, 3, 2, seed=11)
        add = B.random_batch(e.P[:rows], 64, 2, e.np_dtype, 12)
        ks = multipliers(64, 3)
        for a in (None, add):
            assert np.array_equal(e.h_automorphism_mac(ins, ws, ks, addend=a, rows=rows), mac_rns(ins, ws, ks, e.P[:rows], addend=a)), rows


def test_graph_capture_replays_identically(engine_factory):
    """nothing is allocated: the call is captured without a warm-up of its own"""
    import torch
    e = engine_factory(64, 64, 5)
    ins, ws = operands(e, 5, 3, 3, seed=21)
    ks = multipliers(64, 3)
    want = mac_rns(ins, ws, ks, e.P)
    di, dw = [e.to_device(x) for x in ins], [e.to_device(w) for w in ws]
    out = torch.zeros_like(di[0])
    e.automorphism_mac(di, dw, ks, out=out)          # (the module is loaded)
    st, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            e.automorphism_mac(di, dw, ks, out=out, stream=st)
    for _ in range(3):
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(out), want)


def test_invalid_arguments_write_nothing(engine_factory):
    import torch
    from nfllib_amd import _lib
    Lb, ERR = _lib.lib, _lib.ERR_INVALID
    N, nm, batch, terms = 64, 5, 2, 2
    e = engine_factory(64, N, nm)
    x = torch.ones((terms, batch, nm, N), dtype=torch.int64, device="cuda:0")
    w = torch.ones((terms, nm, N), dtype=torch.int64, device="cuda:0")
    o = torch.full((2, batch, nm, N), 9, dtype=torch.int64, device="cuda:0")
    px, pw, po, pa = [x[t].data_ptr() for t in range(terms)], [w[t].data_ptr() for t in range(terms)], o[0].data_ptr(), o[1].data_ptr()
    f, hf = Lb.nflhip_automorphism_mac_dev, Lb.nflhip_automorphism_mac

    def arr(xs, n=17):
        return None if xs is None else (C.c_void_p * n)(*xs)

    def call(ctx=e.ctx, out=po, addend=pa, ins=px, ws=pw, ks=(5, 25), t=terms, b=batch, rows=nm, flags=0, fn=f):
        kv = None if ks is None else (C.c_uint64 * 17)(*ks)
        tail = (None,) if fn is f else ()
        return fn(ctx, out, addend, arr(ins), arr(ws), kv, t, b, rows, flags, *tail)

    assert call(ctx=None) == ERR
    for kw in (dict(out=None), dict(ins=None), dict(ws=None), dict(ks=None), dict(ins=[px[0], None]), dict(ws=[None, pw[1]])):
        assert call(**kw) == ERR, kw                                                      # a NULL pointer (the addend alone may be NULL)
    assert call(t=0) == ERR and call(t=17, ins=(px * 9)[:17], ws=(pw * 9)[:17], ks=(5,) * 17) == ERR
    assert call(rows=0) == ERR and call(rows=nm + 1) == ERR and call(rows=2**64 - 1) == ERR
    for ks in ((4, 5), (5, 0), (5, 2**64 - 2)):
        assert call(ks=ks) == ERR, ks                                                     # an even k
    for flags in (2, 0x100, 0x1000, -1):
        assert call(flags=flags) == ERR, flags
    assert call(b=2**61) == ERR                                                           # the size overflows
    ob, wb = batch * nm * N * 8, nm * N * 8
    for kw in (dict(addend=po + 8), dict(addend=po - ob + 8), dict(out=px[1]), dict(out=px[0] + ob - 8), dict(out=pw[1] - ob + 8),
               dict(out=pw[0] + wb - 8, addend=None), dict(out=px[0], addend=px[0])):
        assert call(**kw) == ERR, kw                                                      # overlaps
    h = [np.ones((batch, nm, N), np.uint64) for _ in range(4)]
    hw = [np.ones((nm, N), np.uint64) for _ in range(2)]
    host = dict(fn=hf, out=h[0].ctypes.data, addend=h[1].ctypes.data, ins=[h[2].ctypes.data, h[3].ctypes.data], ws=[v.ctypes.data for v in hw])
    assert call(**dict(host, out=h[2].ctypes.data)) == ERR and call(**dict(host, ks=(5, 6))) == ERR and call(**dict(host, t=0)) == ERR
    assert call(**dict(host, rows=6)) == ERR and call(**dict(host, ins=None)) == ERR
    assert call(out=None, addend=None, ins=None, ws=None, ks=None, b=0) == 0              # an empty batch is fine
    assert call(fn=hf, out=None, addend=None, ins=None, ws=None, ks=None, b=0) == 0
    torch.cuda.synchronize()
    assert bool((o == 9).all()) and bool((x == 1).all()) and bool((w == 1).all())         # nothing refused above wrote anything
    assert call(ins=[px[0], px[0]], ks=(1, 1), addend=po) == 0                            # ins may repeat, k = 1, the addend in place
    torch.cuda.synchronize()
    assert bool((o[0] == 11).all()) and bool((o[1] == 9).all())
