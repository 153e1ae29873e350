"""GPU: key switching and multiplication below the top level with the ONE top-level key (include/nflhip.h "leveled key switching",
nfllib_amd/csrc/kernels_level.hip).  Every plan, both mod-up modes, both roundings, word for word against tests/level_util.py: the
existing restatements keyswitch_rns / mulrelin_rns on the moduli of the live rows A_l with the gathered key -- the header's
definition of a level call.  No tolerance anywhere.  Inputs are batches of 3, planted per LIVE digit as tests/test_gpu_keyswitch.py
plants them: the edge values, the values around and inside the centred band and every y_i = p_i - 1.  The key is a full top-level
key of uniform words; "dead" are its rows [l, L) and its digits >= dnum_l, which no level-l call may read."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import baseconv_util as B
from keyswitch_util import digits
from level_util import RowsOracle, gather_key, keyswitch_level_rns, level_digits, level_rows, mulrelin_level_rns
from test_gpu_keyswitch import planted

pytestmark = pytest.mark.gpu

KS_PLANS = ("sequence", "composed", "fused")
MR_PLANS = ("sequence", "merged", "fused")
MODES = [(c, f) for c in (False, True) for f in (False, True)]
_CACHE = {}


def level_view(e, K, level):
    """what tests/test_gpu_keyswitch.py planted needs to know of C_l"""
    rows = level_rows(e.nmoduli, K, level)
    return types.SimpleNamespace(P=[e.P[j] for j in rows], nmoduli=len(rows), degree=e.degree, limb_bits=e.limb_bits, np_dtype=e.np_dtype)


def case(e, orc, K, alpha, level, seed=3):
    """the NTT-form inputs over the first l moduli (a1 planted; b1 the NTT form of the constant 1 in polynomials 1 and 2, so that the
    multiplication's d2 is a1 there), the top-level key and, computed on demand and kept, the expected outputs"""
    ck = (e.limb_bits, e.degree, e.nmoduli, K, alpha, level, seed)
    if ck not in _CACHE:
        nm, n = e.nmoduli, e.degree
        dnum = len(digits(nm, K, alpha))
        kept = RowsOracle(orc, nm, range(level))
        ins = [B.random_batch(e.P[:level], n, 3, e.np_dtype, seed + 10 * t) for t in range(4)]
        ins[1] = kept.ntt(planted(level_view(e, K, level), K, alpha, seed))
        ins[3][1:] = 1
        Kk = B.random_batch(e.P, n, 2 * dnum, e.np_dtype, seed + 100).reshape(dnum, 2, nm, n)
        for x in ins + [Kk]:
            x.setflags(write=False)
        _CACHE[ck] = (ins, Kk, {})
    ins, Kk, wants = _CACHE[ck]

    def want_ks(centered, floor):
        k = ("ks", centered, floor)
        if k not in wants:
            wants[k] = keyswitch_level_rns(ins[1], Kk, e.P, K, alpha, level, centered, floor, orc)
        return wants[k]

    def want_mr(centered, floor, rescale, square):
        k = ("mr", centered, floor, rescale, square)
        if k not in wants:
            b = (None, None) if square else (ins[2], ins[3])
            wants[k] = mulrelin_level_rns(ins[0], ins[1], b[0], b[1], Kk, e.P, K, alpha, level, centered, floor, rescale, orc)
        return wants[k]
    return ins, Kk, want_ks, want_mr


def check_ks(e, orc, K, alpha, level, plans=KS_PLANS + (None,), modes=MODES):
    import torch
    ins, Kk, want, _ = case(e, orc, K, alpha, level)
    dA, dK = e.to_device(ins[1]), e.to_device(Kk)
    assert e.keyswitch_digits(K, alpha, level=level) == level_digits(level, alpha)
    for centered, floor in modes:
        w0, w1 = (e.to_device(w) for w in want(centered, floor))
        for plan in plans:
            o0, o1 = e.key_switch_ntt(dA, dK, K, alpha, centered=centered, floor=floor, plan=plan, level=level)
            assert o0.shape == o1.shape == dA.shape == (3, level, e.degree)
            assert torch.equal(o0, w0) and torch.equal(o1, w1), (K, alpha, level, centered, floor, plan)
    assert np.array_equal(e.to_host(dA), ins[1]) and np.array_equal(e.to_host(dK), Kk)


def check_mr(e, orc, K, alpha, level, plans=MR_PLANS + (None,), modes=MODES):
    import torch
    ins, Kk, _, want = case(e, orc, K, alpha, level)
    d, dK = [e.to_device(x) for x in ins], e.to_device(Kk)
    for centered, floor in modes:
        for rescale in (False, True):
            for square in (False, True):
                w0, w1 = (e.to_device(w) for w in want(centered, floor, rescale, square))
                b = (None, None) if square else (d[2], d[3])
                for plan in plans:
                    o0, o1 = e.mul_relin_ntt(d[0], d[1], b[0], b[1], dK, K, alpha, rescale=rescale, centered=centered, floor=floor, plan=plan,
                                             level=level)
                    assert o0.shape == o1.shape == (3, level - 1 if rescale else level, e.degree)
                    assert torch.equal(o0, w0) and torch.equal(o1, w1), (K, alpha, level, centered, floor, rescale, square, plan)
    for x, h in zip(d + [dK], ins + [Kk]):
        assert np.array_equal(e.to_host(x), h)


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 1), (64, 64, 6, 2, 2, 2), (64, 64, 6, 2, 2, 3), (64, 64, 5, 1, 1, 2),
                                                   (32, 128, 4, 1, 1, 1), (32, 128, 4, 1, 1, 2), (64, 64, 20, 2, 1, 17)])
def test_key_switch_every_plan_both_modes_both_roundings(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """u64/64/6 (2, 2): l = 1 has a digit shorter than alpha, l = 2 one digit fewer than the top, l = 3 a short last digit that is full
    at the top (its conversion constants differ from the top-level record's); u64/64/5 (1, 1); u32/128/4: the other limb width, rows
    of 512 bytes; u64/64/20 (2, 1) at l = 17: 17 digits, across the 16-term chunk of dot_reduce.h, the hole right after them"""
    check_ks(engine_factory(lb, n, nm), oracle_factory(lb, n, nm), K, alpha, level)


def test_the_top_level_is_the_existing_entry(engine_factory, oracle_factory):
    """u64/64/6 (2, 2), l = 4 = L: tensor for tensor the output of the call without a level, and the restatement's words"""
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    check_ks(e, orc, 2, 2, 4)
    ins, Kk, _, _ = case(e, orc, 2, 2, 4)
    d, dK = [e.to_device(x) for x in ins], e.to_device(Kk)
    for plan in KS_PLANS + (None,):
        for centered, floor in MODES:
            top = e.key_switch_ntt(d[1], dK, 2, 2, centered=centered, floor=floor, plan=plan)
            lev = e.key_switch_ntt(d[1], dK, 2, 2, centered=centered, floor=floor, plan=plan, level=4)
            assert torch.equal(top[0], lev[0]) and torch.equal(top[1], lev[1]), (plan, centered, floor)
    for plan in MR_PLANS + (None,):
        for rescale in (False, True):
            top = e.mul_relin_ntt(d[0], d[1], d[2], d[3], dK, 2, 2, rescale=rescale, plan=plan)
            lev = e.mul_relin_ntt(d[0], d[1], d[2], d[3], dK, 2, 2, rescale=rescale, plan=plan, level=4)
            assert torch.equal(top[0], lev[0]) and torch.equal(top[1], lev[1]), (plan, rescale)


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 2), (64, 64, 6, 2, 2, 3), (32, 128, 4, 1, 1, 2)])
def test_mul_relin_every_plan_general_and_square_with_and_without_rescale(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    check_mr(engine_factory(lb, n, nm), oracle_factory(lb, n, nm), K, alpha, level)


def test_rescale_at_level_one_and_levels_out_of_range_are_refused(engine_factory, oracle_factory):
    from nfllib_amd import _lib
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    ins, Kk, _, _ = case(e, orc, 2, 2, 1)
    d, dK = [e.to_device(x) for x in ins], e.to_device(Kk)
    o = e.to_device(np.zeros((2, 3, 1, 64), dtype=np.uint64))
    ks, mr = _lib.lib.nflhip_keyswitch_level_ntt_dev, _lib.lib.nflhip_mulrelin_level_ntt_dev
    p = [x.data_ptr() for x in d]
    for level in (0, 5, 2**64 - 1):
        assert ks(e.ctx, o[0].data_ptr(), o[1].data_ptr(), p[1], dK.data_ptr(), 3, 2, 2, level, 0, None) == _lib.ERR_INVALID
        assert mr(e.ctx, o[0].data_ptr(), o[1].data_ptr(), p[0], p[1], p[2], p[3], dK.data_ptr(), 3, 2, 2, level, 0, None) == _lib.ERR_INVALID
        assert _lib.lib.nflhip_keyswitch_level_digits(e.ctx, 2, 2, level) == 0
    assert mr(e.ctx, o[0].data_ptr(), o[1].data_ptr(), p[0], p[1], p[2], p[3], dK.data_ptr(), 3, 2, 2, 1, _lib.MULRELIN_RESCALE, None) == _lib.ERR_INVALID
    assert [_lib.lib.nflhip_keyswitch_level_digits(e.ctx, 2, 2, lv) for lv in (1, 2, 3, 4)] == [1, 1, 2, 2]
    import torch
    torch.cuda.synchronize()
    assert bool((o == 0).all())


def _dead_filled(e, Kk, K, alpha, level, value):
    """the key with rows [l, L) of every polynomial and the digits >= dnum_l set to `value`, truncated after the last live digit: its
    live part ends at the end of the allocation"""
    L, dl = e.nmoduli - K, level_digits(level, alpha)
    k = np.array(Kk)
    k[:, :, level:L] = value
    return np.ascontiguousarray(k[:dl]), k


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 1), (64, 64, 6, 2, 2, 3), (32, 128, 4, 1, 1, 1)])
def test_the_dead_key_is_never_read(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """rows [l, L) and digits >= dnum_l hold all-ones words, which are no canonical residues: every plan returns what it returns with
    zeros there -- the restatement's words, which never saw them.  The key tensor ends with its last live digit, so a read of a
    later digit would leave the allocation."""
    import torch
    e, orc = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    ins, Kk, want_ks, want_mr = case(e, orc, K, alpha, level)
    ones = int(np.iinfo(e.np_dtype).max)
    d = [e.to_device(x) for x in ins]
    for value in (ones, 0):
        short, full = _dead_filled(e, Kk, K, alpha, level, value)
        full[level_digits(level, alpha):] = value
        for key in (e.to_device(short), e.to_device(full)):
            for plan in KS_PLANS + (None,):
                got = e.key_switch_ntt(d[1], key, K, alpha, centered=True, plan=plan, level=level)
                w = want_ks(True, False)
                assert np.array_equal(e.to_host(got[0]), w[0]) and np.array_equal(e.to_host(got[1]), w[1]), (plan, value)
            for plan in MR_PLANS + (None,):
                got = e.mul_relin_ntt(d[0], d[1], d[2], d[3], key, K, alpha, plan=plan, level=level)
                w = want_mr(False, False, False, False)
                assert np.array_equal(e.to_host(got[0]), w[0]) and np.array_equal(e.to_host(got[1]), w[1]), (plan, value)
    torch.cuda.synchronize()


@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 3), (32, 128, 4, 1, 1, 2)])
def test_the_level_call_is_the_level_engine_with_the_gathered_key(lb, n, nm, K, alpha, level, engine_factory, oracle_factory):
    """the definition itself, on the device: Engine.level_engine(l, K) is a context over C_l that this change does not touch otherwise"""
    import torch
    e, orc = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    ins, Kk, _, _ = case(e, orc, K, alpha, level)
    d, dK = [e.to_device(x) for x in ins], e.to_device(Kk)
    c = e.level_engine(level, K)
    try:
        assert c.P == [e.P[j] for j in level_rows(nm, K, level)] == [e.P[j] for j in e.level_rows(level, K)]
        gK = c.to_device(gather_key(Kk, nm, K, alpha, level))
        al = min(alpha, level)
        for centered, floor in MODES:
            a = e.key_switch_ntt(d[1], dK, K, alpha, centered=centered, floor=floor, level=level)
            b = c.key_switch_ntt(d[1], gK, K, al, centered=centered, floor=floor)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            for rescale in (False, True):
                a = e.mul_relin_ntt(d[0], d[1], d[2], d[3], dK, K, alpha, rescale=rescale, centered=centered, floor=floor, level=level)
                b = c.mul_relin_ntt(d[0], d[1], d[2], d[3], gK, K, al, rescale=rescale, centered=centered, floor=floor)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        torch.cuda.synchronize()
    finally:
        c.close()


def test_a_level_fits_the_one_launch_kernel_where_the_top_does_not(engine_factory, oracle_factory):
    """u64/1024/10, K = 1, alpha = 3, batch 1: at l = 9 the (9 + 1) rows of 8 KiB exceed 64 KiB and the forced flag is refused; at l = 7
    the one-launch kernel runs, matches the restatement, and is what the default call chooses.  The words are the same by every plan,
    so the choice is read off the capture rule: only a (plan, modes) that has served this batch may be captured, and after nothing
    but a default call the forced one-launch plan may -- and the composed plan may not."""
    import torch
    from nfllib_amd import Engine, _lib
    orc = oracle_factory(64, 1024, 10)
    e = Engine(64, 1024, 10, device=0)                             # a context of its own: nothing is warm
    try:
        assert (9 + 1) * 1024 * 8 > 65536 >= (7 + 1) * 1024 * 8                    # (fast mode: no corrections in LDS)
        ins, Kk, want, _ = case(e, orc, 1, 3, 7)
        a, dK = e.to_device(ins[1][:1]), e.to_device(Kk)
        a9 = e.to_device(B.random_batch(e.P[:9], 1024, 1, e.np_dtype, 5))
        with pytest.raises(_lib.NflHipError) as err:
            e.key_switch_ntt(a9, dK, 1, 3, plan="fused", level=9)
        assert err.value.code == _lib.ERR_UNSUPPORTED
        w = want(False, False)
        got = e.key_switch_ntt(a, dK, 1, 3, level=7)                # the default
        assert np.array_equal(e.to_host(got[0]), w[0][:1]) and np.array_equal(e.to_host(got[1]), w[1][:1])
        ks = _lib.lib.nflhip_keyswitch_level_ntt_dev
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        o = torch.zeros((2, 1, 7, 1024), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            with torch.cuda.graph(g, stream=st):
                rc_composed = ks(e.ctx, o[0].data_ptr(), o[1].data_ptr(), a.data_ptr(), dK.data_ptr(), 1, 1, 3, 7, _lib.KEYSWITCH_COMPOSED, sp)
                rc_fused = ks(e.ctx, o[0].data_ptr(), o[1].data_ptr(), a.data_ptr(), dK.data_ptr(), 1, 1, 3, 7, _lib.KEYSWITCH_FUSED, sp)
        assert rc_composed == _lib.ERR_UNSUPPORTED and rc_fused == 0
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(o[0]), w[0][:1]) and np.array_equal(e.to_host(o[1]), w[1][:1])
        for plan in ("fused", "composed"):
            got = e.key_switch_ntt(a, dK, 1, 3, plan=plan, level=7)
            assert np.array_equal(e.to_host(got[0]), w[0][:1]) and np.array_equal(e.to_host(got[1]), w[1][:1]), plan
        torch.cuda.synchronize()
    finally:
        e.close()


def test_long_rows(engine_factory, oracle_factory):
    """u64/4096/3, K = alpha = 1, l = 1, batch 2: the composed and merged routes above 2048 words, with the hole"""
    import torch
    e, orc = engine_factory(64, 4096, 3), oracle_factory(64, 4096, 3)
    ins, Kk, want_ks, want_mr = case(e, orc, 1, 1, 1)
    d, dK = [e.to_device(x[:2]) for x in ins], e.to_device(Kk)
    w = want_ks(False, False)
    for plan in ("composed", "sequence", None):
        got = e.key_switch_ntt(d[1], dK, 1, 1, plan=plan, level=1)
        assert np.array_equal(e.to_host(got[0]), w[0][:2]) and np.array_equal(e.to_host(got[1]), w[1][:2]), plan
    w = want_mr(False, False, False, False)
    for plan in ("merged", None):
        got = e.mul_relin_ntt(d[0], d[1], d[2], d[3], dK, 1, 1, plan=plan, level=1)
        assert np.array_equal(e.to_host(got[0]), w[0][:2]) and np.array_equal(e.to_host(got[1]), w[1][:2]), plan
    torch.cuda.synchronize()


# ---- shared behaviour, one case each at u64/64/6 (2, 2), l = 3 ----
def _shared(engine_factory, oracle_factory, seed=3):
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    return (e,) + case(e, orc, 2, 2, 3, seed=seed)


def test_every_buffer_one_word_off_alignment_with_guard_words(engine_factory, oracle_factory):
    import torch
    e, ins, Kk, want, _ = _shared(engine_factory, oracle_factory)
    A = ins[1]
    w0, w1 = want(True, False)
    a = torch.zeros(A.size + 2, dtype=torch.int64, device="cuda:0")
    k = torch.zeros(Kk.size + 2, dtype=torch.int64, device="cuda:0")
    a[1:-1].copy_(e.to_device(A).view(-1)), k[1:-1].copy_(e.to_device(Kk).view(-1))
    for plan in KS_PLANS:
        o0, o1 = (torch.full((A.size + 2,), 7, dtype=torch.int64, device="cuda:0") for _ in range(2))
        e.key_switch_ntt(a[1:-1], k[1:-1], 2, 2, centered=True, out=(o0[1:-1], o1[1:-1]), plan=plan, level=3)
        for o, w in ((o0, w0), (o1, w1)):
            assert np.array_equal(e.to_host(o[1:-1]).reshape(w.shape), w) and int(o[0]) == 7 and int(o[-1]) == 7, plan
    assert int(a[0]) == 0 and int(a[-1]) == 0 and int(k[0]) == 0 and int(k[-1]) == 0


def test_host_variant_equals_device_variant(engine_factory, oracle_factory):
    e, ins, Kk, want_ks, want_mr = _shared(engine_factory, oracle_factory)
    for plan in (None,) + KS_PLANS:
        h0, h1 = e.h_key_switch_ntt(np.array(ins[1]), np.array(Kk), 2, 2, centered=True, plan=plan, level=3)
        d0, d1 = e.key_switch_ntt(e.to_device(ins[1]), e.to_device(Kk), 2, 2, centered=True, plan=plan, level=3)
        w0, w1 = want_ks(True, False)
        assert np.array_equal(h0, w0) and np.array_equal(h1, w1), plan
        assert np.array_equal(e.to_host(d0), h0) and np.array_equal(e.to_host(d1), h1)
    for plan in (None,) + MR_PLANS:
        h0, h1 = e.h_mul_relin_ntt(*[np.array(x) for x in ins], np.array(Kk), 2, 2, rescale=True, plan=plan, level=3)
        w0, w1 = want_mr(False, False, True, False)
        assert np.array_equal(h0, w0) and np.array_equal(h1, w1), plan


@pytest.mark.parametrize("plan", KS_PLANS)
def test_two_streams_share_the_scratch(plan, engine_factory, oracle_factory):
    import torch
    e, ins, Kk, want, _ = _shared(engine_factory, oracle_factory)
    _, ins2, Kk2, want2, _ = _shared(engine_factory, oracle_factory, seed=11)
    dA, dK, dA2, dK2 = (e.to_device(x) for x in (ins[1], Kk, ins2[1], Kk2))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        r1 = e.key_switch_ntt(dA, dK, 2, 2, centered=True, plan=plan, stream=s1, level=3)
        r2 = e.key_switch_ntt(dA2, dK2, 2, 2, centered=True, plan=plan, stream=s2, level=3)
    torch.cuda.synchronize()
    for got, w in ((r1, want(True, False)), (r2, want2(True, False))):
        assert np.array_equal(e.to_host(got[0]), w[0]) and np.array_equal(e.to_host(got[1]), w[1])


@pytest.mark.parametrize("plan", KS_PLANS)
def test_graph_capture_replays_identically(plan, engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up call, then the same call captured and replayed three times"""
    import torch
    e, ins, Kk, want, _ = _shared(engine_factory, oracle_factory)
    w0, w1 = want(True, False)
    dA, dK = e.to_device(ins[1]), e.to_device(Kk)
    both = torch.zeros((2,) + ins[1].shape, dtype=torch.int64, device="cuda:0")
    out = (both[0], both[1])

    def run():
        e.key_switch_ntt(dA, dK, 2, 2, centered=True, out=out, plan=plan, level=3)

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        run()                                                  # the warm-up: the level context, its tables and scratch
        st.synchronize()
        assert np.array_equal(e.to_host(both[0]), w0) and np.array_equal(e.to_host(both[1]), w1)
        with torch.cuda.graph(g, stream=st):
            run()
    for _ in range(3):
        both.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(both[0]), w0) and np.array_equal(e.to_host(both[1]), w1)


def test_first_call_while_capturing_is_refused_and_the_stream_stays_usable(oracle_factory):
    import torch
    from nfllib_amd import Engine, _lib
    e, orc = Engine(64, 64, 6, device=0), oracle_factory(64, 64, 6)   # a context of its own: no level context exists, nothing is warm
    try:
        ins, Kk, want, _ = case(e, orc, 2, 2, 3)
        w0, w1 = want(False, False)
        dA, dK = e.to_device(ins[1]), e.to_device(Kk)
        ks = _lib.lib.nflhip_keyswitch_level_ntt_dev
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        z = torch.zeros(4, device="cuda:0")
        torch.cuda.synchronize()
        for flags in (_lib.KEYSWITCH_FUSED, _lib.KEYSWITCH_COMPOSED, _lib.KEYSWITCH_SEQUENCE):   # (the level context, then each plan, is cold in its turn)
            o = torch.full((2,) + ins[1].shape, 5, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    z.add_(1)
                    rc = ks(e.ctx, o[0].data_ptr(), o[1].data_ptr(), dA.data_ptr(), dK.data_ptr(), 3, 2, 2, 3, flags, sp)
            torch.cuda.synchronize()
            assert rc == _lib.ERR_UNSUPPORTED, (flags, rc)
            assert bool((o == 5).all())                                  # nothing was enqueued
            assert ks(e.ctx, o[0].data_ptr(), o[1].data_ptr(), dA.data_ptr(), dK.data_ptr(), 3, 2, 2, 3, flags, sp) == 0   # the same stream
            st.synchronize()
            assert np.array_equal(e.to_host(o[0]), w0) and np.array_equal(e.to_host(o[1]), w1), flags
    finally:
        e.close()


def test_the_chain_on_the_device(engine_factory, oracle_factory):
    """u64/64/6 (2, 2): mul_relin_ntt(rescale=True, level=l) from l = L = 4 down to 2 with ONE key, each step's result squared by the
    next; the words of every step are the restatement's"""
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    ins, Kk, _, _ = case(e, orc, 2, 2, 4)
    dK = e.to_device(Kk)
    h = (np.array(ins[0]), np.array(ins[1]))
    d = tuple(e.to_device(x) for x in h)
    for level in (4, 3, 2):
        h = mulrelin_level_rns(h[0], h[1], None, None, Kk, e.P, 2, 2, level, False, False, True, orc)
        d = e.mul_relin_ntt(d[0], d[1], None, None, dK, 2, 2, rescale=True, level=level)
        d = tuple(x.contiguous() for x in d)
        assert d[0].shape == (3, level - 1, 64)
        assert np.array_equal(e.to_host(d[0]), h[0]) and np.array_equal(e.to_host(d[1]), h[1]), level


@pytest.fixture(scope="module")
def cpp_program(tmp_path_factory):
    from test_level_cpp import build_cpp
    return build_cpp(str(tmp_path_factory.mktemp("cpp_level")), gpu=True)


@pytest.mark.parametrize("batch", [1, 5])
def test_cpp_surface_on_the_gpu(cpp_program, batch):
    """the program of tests/cpp_level against the real library: poly, poly_p and device_batch equal to the C entries on raw pointers
    with K, the level and the whole key written out, and at the top level to the existing header calls"""
    r = subprocess.run([cpp_program, str(batch)], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
