"""GPU: the weighted sum of NTT-form automorphisms into several outputs (include/nflhip.h "weighted sums of automorphisms into several
outputs"; nfllib_amd/csrc/kernels_bsgs.hip k_permute_mac_multi_ntt), word for word against tests/bsgs_util.py mac_multi_rns -- the
header's formula on Python integers, which is `outputs` times mac_rns.  No tolerance anywhere.  JB = 2 outputs share a launch: the
output counts are 1, JB, JB + 1 (a partial last group) and 16."""
import ctypes as C

import numpy as np
import pytest

import baseconv_util as B
from bsgs_util import mac_multi_rns
from test_gpu_automorphism_mac import multipliers, operands

pytestmark = pytest.mark.gpu
JB = 2
_WANT = {}


def case(e, rows, terms, batch, seed=1):
    """terms inputs, 16 x terms weights of which some are None (output 5 has none at all), addends for the odd outputs; the expected
    words of all 16 outputs, computed once per shape and kept"""
    key = (e.limb_bits, e.degree, e.nmoduli, rows, terms, batch, seed)
    if key not in _WANT:
        ins, _ = operands(e, rows, terms, batch, seed)
        ws = [[None if (o == 5 or (3 * o + t) % 7 == 6) else B.random_batch(e.P, e.degree, 1, e.np_dtype, seed + 200 + 16 * o + t)[0] for t in range(terms)]
              for o in range(16)]
        pm1 = np.array([int(p) - 1 for p in e.P], dtype=e.np_dtype)
        ws[0][0][:, :3] = pm1[:, None]
        adds = [B.random_batch(e.P[:rows], e.degree, batch, e.np_dtype, seed + 900 + o) if o % 2 else None for o in range(16)]
        adds[1][0, :, 0] = pm1[:rows]                                             # the final sum's wrap
        ks = multipliers(e.degree, terms)
        _WANT[key] = (ins, ws, adds, ks, mac_multi_rns(ins, ws, ks, e.P[:rows], addends=adds))
    return _WANT[key]


def check(e, rows, terms, batch, outputs=(1, JB, JB + 1, 16), seed=1):
    ins, ws, adds, ks, want = case(e, rows, terms, batch, seed)
    di = [e.to_device(x) for x in ins]
    dw = [[None if w is None else e.to_device(w) for w in row] for row in ws]
    for no in outputs:
        outs = [e.to_device(np.zeros_like(ins[0])) if a is None else e.to_device(a) for a in adds[:no]]
        got = e.automorphism_mac_multi(di, dw[:no], ks, addends=[None if a is None else o for a, o in zip(adds, outs)], outs=outs, rows=rows)
        for o in range(no):
            assert np.array_equal(e.to_host(got[o]), want[o]), (rows, terms, batch, no, o)
    assert all(np.array_equal(e.to_host(d), h) for d, h in zip(di, ins))          # the inputs are unchanged
    assert all(np.array_equal(e.to_host(d), h) for dr, hr in zip(dw, ws) for d, h in zip(dr, hr) if h is not None)


@pytest.mark.parametrize("rows", [6, 4])
def test_every_output_count_and_term_count(rows, engine_factory):
    """u64/64/6, batch 3: rows = nm and rows = 4 of 6 (the weights keep their nm-row stride); outputs in {1, JB, JB + 1, 16} x terms in
    {1, 2, 16}; NULL weights, an output with none, addends in place; several whole rows per tile, the last tile short"""
    e = engine_factory(64, 64, 6)
    for terms in (1, 2, 16):
        check(e, rows, terms, 3)


@pytest.mark.parametrize("lb,n,nm,terms,batch", [(32, 128, 4, 16, 3), (32, 128, 4, 2, 5), (16, 4, 2, 16, 3)])
def test_other_limb_widths(lb, n, nm, terms, batch, engine_factory):
    """u32/128/4, and u16/4/2 whose rows of 8 bytes take the word variant"""
    check(engine_factory(lb, n, nm), nm, terms, batch)


def test_a_row_of_two_chunks(engine_factory):
    """u64/4096/4, batch 1: a 32 KiB row is two chunks; k = 2n - 1 takes a tile's source from the other chunk, k = 5 from its own"""
    e = engine_factory(64, 4096, 4)
    ins, _ = operands(e, 4, 2, 1, seed=5)
    ws = [[B.random_batch(e.P, 4096, 1, e.np_dtype, 300 + 2 * o + t)[0] for t in range(2)] for o in range(JB + 1)]
    ws[1][0] = None
    ks = [2 * 4096 - 1, 5]
    add = B.random_batch(e.P, 4096, 1, e.np_dtype, 77)
    want = mac_multi_rns(ins, ws, ks, e.P, addends=[None, None, add])
    di, dw = [e.to_device(x) for x in ins], [[None if w is None else e.to_device(w) for w in row] for row in ws]
    outs = [e.to_device(np.zeros_like(add)), e.to_device(np.zeros_like(add)), e.to_device(add)]
    got = e.automorphism_mac_multi(di, dw, ks, addends=[None, None, outs[2]], outs=outs)
    assert all(np.array_equal(e.to_host(g), w) for g, w in zip(got, want))


@pytest.mark.parametrize("lb,n,nm", [(64, 64, 6), (32, 128, 4)])
def test_every_buffer_one_word_off_alignment_with_guard_words(lb, n, nm, engine_factory):
    """the word variant on rows that the 16-byte variant serves otherwise; nothing is written outside the outputs"""
    import torch
    e = engine_factory(lb, n, nm)
    ins, ws, adds, ks, want = case(e, nm, 2, 3)
    no = JB + 1

    def off(h, fill=0):
        t = torch.full((h.size + 2,), fill, dtype=e.torch_dtype, device="cuda:0")
        t[1:-1].copy_(e.to_device(h).view(-1))
        return t
    gi = [off(x) for x in ins]
    gw = [[None if w is None else off(w) for w in row] for row in ws[:no]]
    outs = [torch.full((ins[0].size + 2,), 7, dtype=e.torch_dtype, device="cuda:0") for _ in range(no)]
    for a, o in zip(adds, outs):
        if a is not None:
            o[1:-1].copy_(e.to_device(a).view(-1))
    e.automorphism_mac_multi([t[1:-1] for t in gi], [[None if t is None else t[1:-1] for t in row] for row in gw], ks,
                             addends=[None if a is None else o[1:-1] for a, o in zip(adds, outs)], outs=[o[1:-1] for o in outs])
    for o in range(no):
        assert np.array_equal(e.to_host(outs[o][1:-1]).reshape(want[o].shape), want[o]) and int(outs[o][0]) == 7 and int(outs[o][-1]) == 7, o
    for t, h in zip(gi, ins):
        assert int(t[0]) == 0 and int(t[-1]) == 0 and np.array_equal(e.to_host(t[1:-1]).reshape(h.shape), h)


def test_host_variant_equals_device_variant(engine_factory):
    e = engine_factory(64, 64, 6)
    for rows in (6, 4):
        ins, ws, adds, ks, want = case(e, rows, 2, 3)
        got = e.h_automorphism_mac_multi(ins, ws[:JB + 1], ks, addends=adds[:JB + 1], rows=rows)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), rows


def test_graph_capture_replays_identically(engine_factory):
    """nothing is allocated: the call is captured without a warm-up of its own"""
    import torch
    e = engine_factory(64, 64, 6)
    ins, ws, adds, ks, _ = case(e, 6, 2, 3)
    want = mac_multi_rns(ins, ws[:3], ks, e.P)
    di, dw = [e.to_device(x) for x in ins], [[None if w is None else e.to_device(w) for w in row] for row in ws[:3]]
    outs = [torch.zeros_like(di[0]) for _ in range(3)]
    e.automorphism_mac_multi(di, dw, ks, outs=outs)   # (the module is loaded)
    st, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            e.automorphism_mac_multi(di, dw, ks, outs=outs, stream=st)
    for _ in range(2):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(e.to_host(o), w) for o, w in zip(outs, want))


def test_invalid_arguments_write_nothing(engine_factory):
    """every overlap of an output with an input, a weight or another output; an addend that is not its output; the counts"""
    import torch
    from nfllib_amd import _lib
    f, ERR = _lib.lib.nflhip_automorphism_mac_multi_dev, _lib.ERR_INVALID
    N, nm, batch = 64, 6, 2
    e = engine_factory(64, N, nm)
    x = torch.ones((2, batch, nm, N), dtype=torch.int64, device="cuda:0")
    w = torch.ones((4, nm, N), dtype=torch.int64, device="cuda:0")
    o = torch.full((3, batch, nm, N), 9, dtype=torch.int64, device="cuda:0")
    px, pw, po = [x[t].data_ptr() for t in range(2)], [w[q].data_ptr() for q in range(4)], [o[q].data_ptr() for q in range(2)]
    ob, wb = batch * nm * N * 8, nm * N * 8

    def arr(xs, n=17 * 17):
        return None if xs is None else (C.c_void_p * n)(*xs)

    def call(ctx=e.ctx, outs=po, adds=(None, None), ins=px, ws=pw, ks=(5, 25), no=2, t=2, b=batch, rows=nm, flags=0):
        return f(ctx, arr(outs), arr(adds), arr(ins), arr(ws), None if ks is None else (C.c_uint64 * 17)(*ks), no, t, b, rows, flags, None)
    assert call(ctx=None) == ERR
    for kw in (dict(outs=None), dict(ins=None), dict(ws=None), dict(ks=None), dict(outs=[po[0], None]), dict(ins=[px[0], None])):
        assert call(**kw) == ERR, kw
    assert call(no=0) == ERR and call(no=17) == ERR and call(t=0) == ERR and call(t=17) == ERR
    assert call(rows=0) == ERR and call(rows=nm + 1) == ERR and call(ks=(4, 5)) == ERR and call(flags=1) == ERR and call(b=2**61) == ERR
    for kw in (dict(adds=(po[0] + 8, None)), dict(adds=(po[1], None)), dict(adds=(None, o[2].data_ptr())),      # an addend that is not its output
               dict(outs=[px[1], po[1]]), dict(outs=[po[0], px[0] + ob - 8]),                                  # over an input
               dict(outs=[pw[3] - ob + 8, po[1]]), dict(outs=[po[0], pw[0] + wb - 8]),                          # over a weight
               dict(outs=[po[0], po[0]]), dict(outs=[po[0], po[0] + ob - 8])):                                  # over another output
        assert call(**kw) == ERR, kw
    assert call(outs=None, adds=None, ins=None, ws=None, ks=None, b=0) == 0                # an empty batch is fine
    torch.cuda.synchronize()
    assert bool((o == 9).all()) and bool((x == 1).all()) and bool((w == 1).all())         # nothing refused above wrote anything
    assert call(ws=[pw[0], None, None, None], adds=(po[0], po[1])) == 0                    # NULL weights; the addends in place
    torch.cuda.synchronize()
    assert bool((o[0] == 10).all()) and bool((o[1] == 9).all()) and bool((o[2] == 9).all())
