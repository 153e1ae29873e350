"""GPU: BSGS slot linear transforms (include/nflhip.h "BSGS slot linear transforms"; nfllib_amd/csrc/kernels_bsgs.hip, api.hip
bsgs_run).  Both plans, both mod-up modes, both roundings, word for word against tests/bsgs_util.py: the header's map on Python
integers, at a level through the gathered keys and weights.  No tolerance anywhere.  c1 is a batch of 3 planted per LIVE digit as
tests/test_gpu_level.py plants it; three top-level keys serve as baby and giant keys in turn (keys may repeat), the 16 diagonals of
tests/test_gpu_lintrans.py as weights in turn.  The hoisted plan takes its giant steps in groups of GROUP = 4 and its outputs of the
several-output kernel two per launch."""
import ctypes as C

import numpy as np
import pytest

import baseconv_util as B
from bsgs_util import bsgs_level_rns
from keyswitch_util import digits
from level_rotate_util import gather_weight
from level_util import RowsOracle, gather_key, level_digits
from test_gpu_keyswitch import planted
from test_gpu_level import level_view
from test_gpu_lintrans import diagonals

pytestmark = pytest.mark.gpu

GROUP = 4
PLANS = ("sequence", "hoisted")
MODES = [(c, f) for c in (False, True) for f in (False, True)]
PICK = {1: [0], 3: [0, 1, 2], 5: [0, 1, 2, 0, 1]}
SHAPES = [(64, 64, 6, 2, 2, 1), (64, 64, 6, 2, 2, 3), (64, 64, 6, 2, 2, 4), (64, 64, 5, 2, 1, 2), (32, 128, 4, 1, 1, 1), (32, 128, 4, 1, 1, 2),
          (64, 64, 20, 2, 1, 9)]
# (n1, n2, unkeyed babies, unkeyed giants, (j, i) of the NULL weights)
MIXED, ALL_KEYED, BOUNDARY = (3, 3, (1,), (0,), ()), (3, 3, (), (), ()), (2, GROUP + 1, (), (), ())
STEPS = [(1, 1, (), (), ()), MIXED, ALL_KEYED, (16, 2, (3,), (), ()), (2, 16, (), (7,), ()), BOUNDARY,
         (3, 3, (0,), (2,), ((0, 0), (0, 1), (1, 1), (1, 2), (2, 0))), (1, 2, (0,), (1,), ()), (2, 2, (0, 1), (), ())]
_CACHE = {}


def steps(n, n1, n2, ub, ug, nulls, ws):
    """(bks, index of the key or None), (gks, index or None), weights[j][i]: distinct odd multipliers, the three keys in turn"""
    bks = [1 if i in ub else pow(5, i + 1, 2 * n) for i in range(n1)]
    bw = [None if i in ub else i % 3 for i in range(n1)]
    gks = [2 * n + 1 if j in ug else (2 * n - 1) * pow(5, 2 * j, 2 * n) % (2 * n) for j in range(n2)]
    gw = [None if j in ug else (j + 1) % 3 for j in range(n2)]
    weights = [[None if (j, i) in nulls else ws[(j * n1 + i) % 16] for i in range(n1)] for j in range(n2)]
    return bks, bw, gks, gw, weights


def case(e, orc, K, alpha, level, seed=3, polys=3):
    """c0, c1 = [polys, l, n] in NTT form (c1 planted per live digit), three TOP-LEVEL keys, the 16 top-level diagonals and, computed on
    demand and kept, the expected words"""
    ck = (e.limb_bits, e.degree, e.nmoduli, K, alpha, level, seed, polys)
    if ck not in _CACHE:
        nm, n = e.nmoduli, e.degree
        dnum = len(digits(nm, K, alpha))
        kept = RowsOracle(orc, nm, range(level))
        c1 = kept.ntt(planted(level_view(e, K, level), K, alpha, seed)[:polys])
        c0 = B.random_batch(e.P[:level], n, polys, e.np_dtype, seed + 50)
        c0[0, :, :2] = np.array([int(p) - 1 for p in e.P[:level]], dtype=e.np_dtype)[:, None]      # the sum's wrap: p - 1 + anything
        c0[-1, :, -1] = 0
        keys = [B.random_batch(e.P, n, 2 * dnum, e.np_dtype, seed + 100 + i).reshape(dnum, 2, nm, n) for i in range(3)]
        for x in [c0, c1] + keys:
            x.setflags(write=False)
        _CACHE[ck] = (c0, c1, keys, {}, {})
    c0, c1, keys, memo, wants = _CACHE[ck]
    ws = diagonals(e)

    def want(centered, floor, st, with_c0=True, pick=None):
        wk = (centered, floor, st, with_c0)
        if wk not in wants:
            bks, bw, gks, gw, weights = steps(e.degree, *st, ws)
            wants[wk] = bsgs_level_rns(c0 if with_c0 else None, c1, [None if i is None else keys[i] for i in bw], bks,
                                       [None if i is None else keys[i] for i in gw], gks, weights, e.P, K, alpha, level, centered, floor, orc,
                                       memo=memo.setdefault(centered, {}))
        r = wants[wk]
        return r if pick is None else (r[0][pick], r[1][pick])
    return c0, c1, keys, ws, want


def run(e, dc0, dc1, dkeys, dws, st, K, alpha, level, **kw):
    bks, bw, gks, gw, weights = steps(e.degree, *st, dws)
    return e.bsgs_linear_transform_ntt(dc0, dc1, [None if i is None else dkeys[i] for i in bw], bks, [None if i is None else dkeys[i] for i in gw], gks,
                                       weights, K, alpha, level=level, **kw)


def same(e, got, want):
    return all(np.array_equal(e.to_host(got[c]).reshape(want[c].shape), want[c]) for c in (0, 1))


def check(e, orc, K, alpha, level, modes, cases, batch=3, plans=PLANS):
    """the entry over the step counts x modes x plans; the inputs, keys and weights are unchanged afterwards"""
    c0, c1, keys, ws, want = case(e, orc, K, alpha, level)
    pick = PICK[batch]
    dc0, dc1, dkeys, dws = e.to_device(c0[pick]), e.to_device(c1[pick]), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    for st in cases:
        for centered, floor in modes:
            w = want(centered, floor, st, pick=pick)
            for plan in plans:
                got = run(e, dc0, dc1, dkeys, dws, st, K, alpha, level, centered=centered, floor=floor, plan=plan)
                assert got[0].shape == got[1].shape == dc1.shape == (batch, level, e.degree)
                assert same(e, got, w), (K, alpha, level, st, batch, centered, floor, plan)
    assert np.array_equal(e.to_host(dc0), c0[pick]) and np.array_equal(e.to_host(dc1), c1[pick])
    assert all(np.array_equal(e.to_host(d), h) for d, h in zip(dkeys + dws, keys + ws))


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", SHAPES)
def test_every_shape_both_plans_both_modes_both_roundings(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """u64/64/6 (2, 2): l = 1 has a digit shorter than alpha, l = 3 a short last digit, l = 4 is the top; u64/64/5 (2, 1); u32/128/4: the
    other limb width; u64/64/20 (2, 1), l = 9: the streaming form of k_dot_multi.  Batch 3.  (3, 3) with one unkeyed baby and one
    unkeyed giant, and (2, GROUP + 1): a group boundary and a partial output group.  Rows of 512 bytes put 32 rows in a tile of the
    several-output kernel, so every tile here straddles the split: the per-item weight select."""
    check(engine_factory(lb, n, nm), oracle_factory(lb, n, nm), K, alpha, level, MODES, [MIXED, BOUNDARY])


@pytest.mark.parametrize("st", STEPS)
def test_every_step_count(st, engine_factory, oracle_factory):
    """u64/64/6 (2, 2), l = 3, batch 3, every mode and plan: (1, 1); (3, 3) mixed and all keyed; (16, 2); (2, 16) and (2, GROUP + 1); NULL
    weights (a giant step whose only weight is on the unkeyed baby, another with none on it); unkeyed babies only"""
    check(engine_factory(64, 64, 6), oracle_factory(64, 64, 6), 2, 2, 3, MODES, [st])


@pytest.mark.parametrize("batch", [1, 5])
def test_batch_one_and_five(batch, engine_factory, oracle_factory):
    check(engine_factory(64, 64, 6), oracle_factory(64, 64, 6), 2, 2, 3, [(False, False), (True, True)], [MIXED, BOUNDARY], batch=batch)


def test_c0_null_and_output_placement(engine_factory, oracle_factory):
    """c0 = None, with and without a keyed step; out1 adjacent to out0 (one mod-down call) and apart from it"""
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    c0, c1, keys, ws, want = case(e, orc, 2, 2, 3)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    for plan in PLANS:
        for st in (MIXED, (2, 2, (0, 1), (), ()), (2, 2, (0, 1), (0, 1), ())):
            assert same(e, run(e, None, dc1, dkeys, dws, st, 2, 2, 3, centered=True, plan=plan), want(True, False, st, with_c0=False)), (plan, st)
        w = want(False, True, MIXED)
        apart = torch.zeros((3,) + c1.shape, dtype=torch.int64, device="cuda:0")
        assert same(e, run(e, dc0, dc1, dkeys, dws, MIXED, 2, 2, 3, floor=True, plan=plan, out=(apart[2], apart[0])), w), plan
        assert bool((apart[1] == 0).all())


def test_a_row_of_two_chunks(engine_factory, oracle_factory):
    """u64/4096/4, K = 1, l = 2, batch 1: a 32 KiB row is two chunks, the per-tile weight select; k = 2n - 1 takes a tile's source from
    the other chunk, k = 5 from its own.  The hoisted mod-up takes the inverse-transform route here."""
    e, orc = engine_factory(64, 4096, 4), oracle_factory(64, 4096, 4)
    c0, c1, keys, ws, _ = case(e, orc, 1, 1, 2, polys=1)
    bks, gks = [5, 1], [2 * 4096 - 1, 1, 25]
    bkeys, gkeys = [keys[0], None], [keys[1], None, keys[2]]
    weights = [[ws[2 * j + i] for i in range(2)] for j in range(3)]
    dkeys, dws = [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:6]]
    dc0, dc1 = e.to_device(c0), e.to_device(c1)
    for centered, floor in ((False, False), (True, True)):
        w = bsgs_level_rns(c0, c1, bkeys, bks, gkeys, gks, weights, e.P, 1, 1, 2, centered, floor, orc)
        for plan in PLANS:
            got = e.bsgs_linear_transform_ntt(dc0, dc1, [dkeys[0], None], bks, [dkeys[1], None, dkeys[2]], gks,
                                              [[dws[2 * j + i] for i in range(2)] for j in range(3)], 1, 1, centered=centered, floor=floor, plan=plan, level=2)
            assert same(e, got, w), (centered, floor, plan)


def test_one_unkeyed_giant_step_is_the_linear_transform_on_the_device(engine_factory, oracle_factory):
    """n2 = 1 with the unrotated giant step: tensor for tensor linear_transform_ntt(level=)"""
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    ks, which = [5, 1, 25, 2 * 64 - 1], [0, None, 1, 2]
    for level in (3, 4):
        c0, c1, keys, ws, _ = case(e, orc, 2, 2, level)
        a0, a1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws[:4]]
        lk = [None if i is None else dkeys[i] for i in which]
        for centered, floor in MODES:
            lt = e.linear_transform_ntt(a0, a1, lk, dws, ks, 2, 2, centered=centered, floor=floor, level=level)
            for plan in PLANS:
                got = e.bsgs_linear_transform_ntt(a0, a1, lk, ks, [None], [1], [dws], 2, 2, centered=centered, floor=floor, plan=plan, level=level)
                assert torch.equal(got[0], lt[0]) and torch.equal(got[1], lt[1]), (level, centered, floor, plan)
    top = e.bsgs_linear_transform_ntt(a0, a1, lk, ks, [None], [1], [dws], 2, 2, centered=True, floor=True)     # no level: the top
    assert torch.equal(top[0], got[0]) and torch.equal(top[1], got[1])


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 3), (64, 64, 6, 2, 2, 1), (32, 128, 4, 1, 1, 2)])
def test_the_level_call_is_the_level_engine_with_gathered_keys_and_weights(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """the definition itself, on the device: Engine.level_engine(l, K) is a context over C_l, on which the call is a top-level one"""
    import torch
    e, orc = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    c0, c1, keys, ws, _ = case(e, orc, K, alpha, level)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(w) for w in ws]
    c = e.level_engine(level, K)
    try:
        gk = [c.to_device(gather_key(k, nm, K, alpha, level)) for k in keys]
        gw = [c.to_device(gather_weight(w, nm, K, level)) for w in ws]
        for st in (MIXED, BOUNDARY):
            for plan in PLANS:
                for centered, floor in ((False, False), (True, True)):
                    a = run(e, dc0, dc1, dkeys, dws, st, K, alpha, level, centered=centered, floor=floor, plan=plan)
                    b = run(c, dc0, dc1, gk, gw, st, K, min(alpha, level), None, centered=centered, floor=floor, plan=plan)
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (st, plan, centered, floor)
        torch.cuda.synchronize()
    finally:
        c.close()


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 1), (64, 64, 6, 2, 2, 3), (32, 128, 4, 1, 1, 1)])
def test_dead_rows_and_digits_are_never_read(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """rows [l, L) of every key and weight and the digits >= dnum_l of every key hold all-ones words (no canonical residues), then
    zeros: both plans return the restatement's words, which never saw them.  A key cut after its last live digit is accepted."""
    import torch
    e, orc = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    c0, c1, keys, ws, want = case(e, orc, K, alpha, level)
    L, dl, ones = nm - K, level_digits(level, alpha), int(np.iinfo(e.np_dtype).max)
    dc0, dc1 = e.to_device(c0), e.to_device(c1)
    w = want(True, False, MIXED)
    for value in (ones, 0):
        full, cut, dws = [], [], []
        for k in keys:
            k = np.array(k)
            k[:, :, level:L] = value
            k[dl:] = value
            full.append(e.to_device(k))
            cut.append(e.to_device(np.ascontiguousarray(k[:dl])))
        for x in ws:
            x = np.array(x)
            x[level:L] = value
            dws.append(e.to_device(x))
        for dkeys in (full, cut):
            for plan in PLANS:
                assert same(e, run(e, dc0, dc1, dkeys, dws, MIXED, K, alpha, level, centered=True, plan=plan), w), (plan, value)
    torch.cuda.synchronize()


def test_every_buffer_one_word_off_alignment_with_guard_words(engine_factory, oracle_factory):
    """the word variants of the kernels, with the hole; nothing is written outside the outputs"""
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    c0, c1, keys, ws, want = case(e, orc, 2, 2, 3)
    w = want(True, False, MIXED)

    def off(h, fill=0):
        t = torch.full((h.size + 2,), fill, dtype=torch.int64, device="cuda:0")
        t[1:-1].copy_(e.to_device(h).view(-1))
        return t
    a0, a1, ak, aw = off(c0), off(c1), [off(k) for k in keys], [off(x) for x in ws]
    for plan in PLANS:
        o = tuple(torch.full((c1.size + 2,), 7, dtype=torch.int64, device="cuda:0") for _ in range(2))
        run(e, a0[1:-1].view(c0.shape), a1[1:-1].view(c1.shape), [k[1:-1] for k in ak], [x[1:-1] for x in aw], MIXED, 2, 2, 3, centered=True,
            out=(o[0][1:-1], o[1][1:-1]), plan=plan)
        for c in (0, 1):
            assert np.array_equal(e.to_host(o[c][1:-1]).reshape(w[c].shape), w[c]) and int(o[c][0]) == 7 and int(o[c][-1]) == 7, plan
    for t, h in [(a0, c0), (a1, c1)] + list(zip(ak, keys)) + list(zip(aw, ws)):
        assert int(t[0]) == 0 and int(t[-1]) == 0 and np.array_equal(e.to_host(t[1:-1]).reshape(h.shape), h)


def test_host_variant_equals_device_variant(engine_factory, oracle_factory):
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    c0, c1, keys, ws, want = case(e, orc, 2, 2, 3)
    st = (3, 3, (0,), (2,), ((0, 1), (2, 0)))
    bks, bw, gks, gw, weights = steps(64, *st, ws)
    for plan in PLANS:
        h = e.h_bsgs_linear_transform_ntt(np.array(c0), np.array(c1), [None if i is None else keys[i] for i in bw], bks,
                                          [None if i is None else keys[i] for i in gw], gks, weights, 2, 2, centered=True, plan=plan, level=3)
        w = want(True, False, st)
        assert np.array_equal(h[0], w[0]) and np.array_equal(h[1], w[1]), plan


@pytest.mark.parametrize("plan", PLANS)
def test_two_streams_share_the_scratch(plan, engine_factory, oracle_factory):
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    c0, c1, keys, ws, want = case(e, orc, 2, 2, 3)
    b0, b1, keys2, _, want2 = case(e, orc, 2, 2, 3, seed=11)
    d = [e.to_device(x) for x in (c0, c1, b0, b1)]
    dk, dk2, dws = [e.to_device(k) for k in keys], [e.to_device(k) for k in keys2], [e.to_device(w) for w in ws]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        r1 = run(e, d[0], d[1], dk, dws, MIXED, 2, 2, 3, centered=True, plan=plan, stream=s1)
        r2 = run(e, d[2], d[3], dk2, dws, MIXED, 2, 2, 3, centered=True, plan=plan, stream=s2)
    torch.cuda.synchronize()
    assert same(e, r1, want(True, False, MIXED)) and same(e, r2, want2(True, False, MIXED))


@pytest.mark.parametrize("plan", PLANS)
def test_graph_capture_replays_identically(plan, engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up call, then the same call captured and replayed three times"""
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    c0, c1, keys, ws, want = case(e, orc, 2, 2, 3)
    w = want(True, False, BOUNDARY)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(x) for x in ws]
    out = torch.zeros((2,) + c1.shape, dtype=torch.int64, device="cuda:0")

    def go():
        run(e, dc0, dc1, dkeys, dws, BOUNDARY, 2, 2, 3, centered=True, plan=plan, out=(out[0], out[1]), stream=st)
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        go()                                                   # the warm-up: the level context, its tables and scratch
        st.synchronize()
        assert same(e, out, w)
        with torch.cuda.graph(g, stream=st):
            go()
    for _ in range(3):
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(e, out, w)


def _raw(e, lib, o0, o1, p0, p1, dkeys, dws, st, batch, K, alpha, level, flags, stream):
    bks, bw, gks, gw, weights = steps(e.degree, *st, dws)
    n1, n2 = len(bks), len(gks)
    pb = (C.c_void_p * n1)(*[None if i is None else dkeys[i].data_ptr() for i in bw])
    pg = (C.c_void_p * n2)(*[None if i is None else dkeys[i].data_ptr() for i in gw])
    pw = (C.c_void_p * (n1 * n2))(*[None if x is None else x.data_ptr() for row in weights for x in row])
    return lib.nflhip_bsgs_ntt_dev(e.ctx, o0, o1, p0, p1, pb, (C.c_uint64 * n1)(*bks), n1, pg, (C.c_uint64 * n2)(*gks), n2, pw, batch, K, alpha, level,
                                   flags, stream)


def test_first_call_while_capturing_is_refused_and_the_stream_stays_usable(oracle_factory):
    import torch
    from nfllib_amd import Engine, _lib
    e, orc = Engine(64, 64, 6, device=0), oracle_factory(64, 64, 6)   # a context of its own: no level context exists, nothing is warm
    try:
        c0, c1, keys, ws, want = case(e, orc, 2, 2, 3)
        w = want(False, False, MIXED)
        dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(x) for x in ws]
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        z = torch.zeros(4, device="cuda:0")
        o = torch.full((2, 3, 3, 64), 5, dtype=torch.int64, device="cuda:0")
        for flags in (_lib.BSGS_HOISTED, _lib.BSGS_SEQUENCE):                     # (the level context, then each plan, is cold in its turn)
            def call():
                return _raw(e, _lib.lib, o[0].data_ptr(), o[1].data_ptr(), dc0.data_ptr(), dc1.data_ptr(), dkeys, dws, MIXED, 3, 2, 2, 3, flags, sp)
            o.fill_(5)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    z.add_(1)
                    rc = call()
            torch.cuda.synchronize()
            assert rc == _lib.ERR_UNSUPPORTED, (flags, rc)
            assert bool((o == 5).all())                                  # nothing was enqueued
            assert call() == 0                                          # the same stream
            st.synchronize()
            assert same(e, (o[0], o[1]), w), flags
    finally:
        e.close()


def test_invalid_arguments(engine_factory, oracle_factory):
    """n1 or n2 of 0 or 17, an even k, a NULL key with k != 1, a giant step with no weight, two plan flags, level 0 or L + 1, an output
    over an input, a key or a weight: NFLHIP_ERR_INVALID, nothing written"""
    import torch
    from nfllib_amd import _lib
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    c0, c1, keys, ws, _ = case(e, orc, 2, 2, 3)
    dc0, dc1, dkeys, dws = e.to_device(c0), e.to_device(c1), [e.to_device(k) for k in keys], [e.to_device(x) for x in ws]
    o = torch.zeros((2,) + c1.shape, dtype=torch.int64, device="cuda:0")
    f, bad = _lib.lib.nflhip_bsgs_ntt_dev, _lib.ERR_INVALID

    def arr(xs):
        return (C.c_void_p * 17)(*xs)

    def call(o0=o[0].data_ptr(), o1=o[1].data_ptr(), p0=dc0.data_ptr(), bkeys=(dkeys[0].data_ptr(), None), bks=(5, 1), n1=2,
             gkeys=(dkeys[1].data_ptr(), None), gks=(25, 1), n2=2, weights=None, level=3, flags=0):
        weights = [dws[q].data_ptr() for q in range(4)] if weights is None else weights
        return f(e.ctx, o0, o1, p0, dc1.data_ptr(), arr(list(bkeys)), (C.c_uint64 * 17)(*bks), n1, arr(list(gkeys)), (C.c_uint64 * 17)(*gks), n2,
                 (C.c_void_p * 289)(*weights), 3, 2, 2, level, flags, None)
    assert call() == 0
    torch.cuda.synchronize()
    o.zero_()
    for kw in (dict(n1=0), dict(n1=17), dict(n2=0), dict(n2=17), dict(bks=(4, 1)), dict(gks=(25, 2)), dict(bks=(5, 3)), dict(gks=(25, 7)),
               dict(weights=[dws[0].data_ptr(), dws[1].data_ptr(), None, None]), dict(flags=_lib.BSGS_SEQUENCE | _lib.BSGS_HOISTED), dict(flags=1),
               dict(level=0), dict(level=5), dict(level=2**64 - 1), dict(o0=dc0.data_ptr()), dict(o1=dc1.data_ptr()), dict(o1=o[0].data_ptr() + 8),
               dict(o0=dkeys[1][1, 1, 3].data_ptr()), dict(o1=dws[3][3:].data_ptr())):
        assert call(**kw) == bad, kw
    torch.cuda.synchronize()
    assert bool((o == 0).all()) and np.array_equal(e.to_host(dc1), c1) and np.array_equal(e.to_host(dkeys[1]), keys[1])
    assert call(weights=[dws[0].data_ptr(), None, None, dws[1].data_ptr()]) == 0       # NULL weights, every giant step with one
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cpp_program(tmp_path_factory):
    from test_bsgs_cpp import build_cpp
    return build_cpp(str(tmp_path_factory.mktemp("cpp_bsgs")), gpu=True)


@pytest.mark.parametrize("batch", [1, 5])
def test_cpp_surface_on_the_gpu(cpp_program, batch):
    """the program of tests/cpp_bsgs against the real library: poly, poly_p and device_batch equal to the C entry on raw pointers with
    the baby keys, the giant keys, the diagonals at j * n1 + i, K and the level written out"""
    import os
    import subprocess
    r = subprocess.run([cpp_program, str(batch)], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
