"""GPU: sums of ciphertext products with one relinearisation (include/nflhip.h "sums of ciphertext products").
Every plan, both mod-up modes, both roundings, with and without the rescale, general and square, dense and shared b, word for word
against tests/mulrelin_dot_util.mulrelin_dot_rns; without the rescale also against D_c + key_switch_ntt(D2) through the engine's own
entries.  No tolerance anywhere.  The reference of a (shape, level, terms) is computed once, for three groups; one group is its
group 0."""
import ctypes as C

import numpy as np
import pytest

import baseconv_util as B
from keyswitch_util import digits
from level_util import mulrelin_level_rns
from mulrelin_dot_util import mulrelin_dot_rns, operand

pytestmark = pytest.mark.gpu

PLANS = ("sequence", "merged", None)
MODES = [(c, f) for c in (False, True) for f in (False, True)]
_CACHE = {}


def case(e, orc, K, alpha, level, terms, seed=3):
    """3 groups of `terms` uniform ciphertext pairs over the first `level` moduli, a uniform top-level key, and the expected outputs
    computed on demand and kept"""
    ck = (e.limb_bits, e.degree, e.nmoduli, K, alpha, level, terms, seed)
    if ck not in _CACHE:
        nm, n = e.nmoduli, e.degree
        dnum = len(digits(nm, K, alpha))
        ins = [B.random_batch(e.P[:level], n, 3 * terms, e.np_dtype, seed + 10 * t) for t in range(4)]
        for m in range(level):                                                   # the largest words in group 0
            ins[0][0, m] = ins[1][0, m] = ins[2][0, m] = ins[3][0, m] = e.P[m] - 1
        Kk = B.random_batch(e.P, n, 2 * dnum, e.np_dtype, seed + 100).reshape(dnum, 2, nm, n)
        for x in ins + [Kk]:
            x.setflags(write=False)
        _CACHE[ck] = (ins, Kk, {})
    ins, Kk, wants = _CACHE[ck]

    def want(centered, floor, rescale, square, shared):
        k = (centered, floor, rescale, square, shared)
        if k not in wants:
            a0, a1 = operand(ins[0], 3, terms), operand(ins[1], 3, terms)
            b = (None, None) if square else tuple(operand(x[:terms] if shared else x, 3, terms, shared) for x in ins[2:])
            wants[k] = mulrelin_dot_rns(a0, a1, b[0], b[1], Kk, e.P, K, alpha, level, centered, floor, rescale, orc)
        return wants[k]
    return ins, Kk, want


def device_operands(e, ins, groups, terms, shared):
    d = [e.to_device(x[:groups * terms]) for x in ins[:2]]
    d += [e.to_device(x[:terms] if shared else x[:groups * terms]) for x in ins[2:]]
    return d


def check(e, el, orc, K, alpha, level, terms, groups):
    import torch
    from nfllib_amd import _lib
    ins, Kk, want = case(e, orc, K, alpha, level, terms)
    dK = e.to_device(Kk)
    for shared in (False, True):
        d = device_operands(e, ins, groups, terms, shared)
        for square in ((False, True) if not shared else (False,)):
            b = (None, None) if square else (d[2], d[3])
            plans = PLANS + (("fused",) if terms == 1 and (not shared or groups == 1) else ())
            for centered, floor in MODES:
                for rescale in ((False, True) if level >= 2 else (False,)):
                    w0, w1 = (e.to_device(w[:groups]) for w in want(centered, floor, rescale, square, shared))
                    for plan in plans:
                        o0, o1 = e.mul_relin_dot_ntt(d[0], d[1], b[0], b[1], terms, dK, K, alpha, b_shared=shared, rescale=rescale,
                                                     centered=centered, floor=floor, plan=plan, level=level)
                        assert o0.shape == o1.shape == (groups, level - 1 if rescale else level, e.degree)
                        assert torch.equal(o0, w0) and torch.equal(o1, w1), (level, terms, groups, shared, square, centered, floor, rescale, plan)
                    if not rescale:                                              # identity 1 through the engine's own entries
                        D = e.tensor_dot_ntt(d[0], d[1], b[0], b[1], terms=terms, rows=level, b_shared=shared)
                        k0, k1 = e.key_switch_ntt(D[2].contiguous(), dK, K, alpha, centered=centered, floor=floor, level=level)
                        assert torch.equal(el.pointwise(_lib.OP_ADD, D[0].contiguous(), k0), w0)
                        assert torch.equal(el.pointwise(_lib.OP_ADD, D[1].contiguous(), k1), w1)
        for x, h in zip(d, ins):
            assert np.array_equal(e.to_host(x), h[:x.shape[0]])                  # the operands are only read


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("terms", [1, 2, 9, 17])
@pytest.mark.parametrize("lb,n,nm,K,alpha,level", [(64, 64, 6, 2, 2, 4), (64, 64, 6, 2, 2, 3), (64, 64, 6, 2, 2, 2), (32, 128, 4, 1, 1, 3),
                                                   (32, 128, 4, 1, 1, 2)])
def test_every_plan_mode_rounding_rescale_square_and_layout(lb, n, nm, K, alpha, level, terms, groups, engine_factory, oracle_factory):
    """u64/64/6 (2, 2) at the top level 4, at 3 (a short last digit) and at 2 (one digit fewer); u32/128/4 (1, 1) at the top level 3
    and at 2.  terms 9 and 17 cross the two reduction cadences of the kernel; the sequence crosses the 16-term chunk of k_dot."""
    check(engine_factory(lb, n, nm), engine_factory(lb, n, level), oracle_factory(lb, n, nm), K, alpha, level, terms, groups)


@pytest.mark.parametrize("level", [4, 2])
def test_one_term_of_dense_operands_is_the_multiplication(level, engine_factory, oracle_factory):
    """tensor for tensor the output of mul_relin_ntt(level=...), under every plan, the one-launch kernel included"""
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    ins, Kk, _ = case(e, orc, 2, 2, level, 1)
    d, dK = [e.to_device(x) for x in ins], e.to_device(Kk)
    for plan in ("sequence", "merged", "fused", None):
        for rescale in (False, True):
            for b in ((d[2], d[3]), (None, None)):
                one = e.mul_relin_ntt(d[0], d[1], b[0], b[1], dK, 2, 2, rescale=rescale, centered=True, plan=plan, level=level)
                dot = e.mul_relin_dot_ntt(d[0], d[1], b[0], b[1], 1, dK, 2, 2, rescale=rescale, centered=True, plan=plan, level=level)
                assert torch.equal(one[0], dot[0]) and torch.equal(one[1], dot[1]), (plan, rescale, b[0] is None)


def test_the_one_launch_plan_is_refused_for_more_than_one_term(engine_factory, oracle_factory):
    from nfllib_amd import _lib
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    ins, Kk, want = case(e, orc, 2, 2, 4, 2)
    d, dK = device_operands(e, ins, 3, 2, False), e.to_device(Kk)
    with pytest.raises(_lib.NflHipError) as err:
        e.mul_relin_dot_ntt(*d, 2, dK, 2, 2, plan="fused")
    assert err.value.code == _lib.ERR_UNSUPPORTED
    got = e.mul_relin_dot_ntt(*d, 2, dK, 2, 2)                                  # and the context goes on serving
    w = want(False, False, False, False, False)
    assert np.array_equal(e.to_host(got[0]), w[0]) and np.array_equal(e.to_host(got[1]), w[1])


@pytest.mark.parametrize("level", [1, 2])
def test_long_rows_take_the_composed_mod_up(level, engine_factory, oracle_factory):
    """u64/4096/3, K = alpha = 1, 2 groups of 3 terms: above 2048 words the merged plan inverse-transforms D2 once and runs
    k_modup_digits.  Level 1 is below the top; level 2, the top, with the rescale."""
    import torch
    e, orc = engine_factory(64, 4096, 3), oracle_factory(64, 4096, 3)
    n, groups, terms, rescale = 4096, 2, 3, level == 2
    ins = [B.random_batch(e.P[:level], n, groups * terms, np.uint64, 60 + t) for t in range(4)]
    Kk = B.random_batch(e.P, n, 4, np.uint64, 70).reshape(2, 2, 3, n)
    w = mulrelin_dot_rns(*[operand(x, groups, terms) for x in ins], Kk, e.P, 1, 1, level, True, False, rescale, orc)
    d, dK = [e.to_device(x) for x in ins], e.to_device(Kk)
    for plan in PLANS:
        got = e.mul_relin_dot_ntt(*d, terms, dK, 1, 1, rescale=rescale, centered=True, plan=plan, level=level)
        assert np.array_equal(e.to_host(got[0]), w[0]) and np.array_equal(e.to_host(got[1]), w[1]), (level, plan)


def test_an_output_that_is_exactly_operand_zero(engine_factory, oracle_factory):
    """out0 begins at a0's first byte and out1 at b1's: every read is enqueued before the mod-down writes.  One word further on is
    refused."""
    import torch
    from nfllib_amd import _lib
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    groups, terms, level = 3, 2, 4
    ins, Kk, want = case(e, orc, 2, 2, level, terms)
    w = want(True, False, False, False, False)
    dK = e.to_device(Kk)
    for plan in PLANS:
        d = device_operands(e, ins, groups, terms, False)
        e.mul_relin_dot_ntt(*d, terms, dK, 2, 2, centered=True, plan=plan, out=(d[0][:groups], d[3][:groups]))
        assert np.array_equal(e.to_host(d[0][:groups]), w[0]) and np.array_equal(e.to_host(d[3][:groups]), w[1]), plan
    d = device_operands(e, ins, groups, terms, False)
    other = torch.empty((groups, level, 64), dtype=torch.int64, device="cuda:0")
    with pytest.raises(_lib.NflHipError) as err:
        e.mul_relin_dot_ntt(*d, terms, dK, 2, 2, out=(d[0].view(-1)[1:1 + groups * level * 64].view(groups, level, 64), other))
    assert err.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.NflHipError) as err:                                 # inside an operand's extent, not at its start
        e.mul_relin_dot_ntt(*d, terms, dK, 2, 2, out=(other, d[1][1:1 + groups]))
    assert err.value.code == _lib.ERR_INVALID
    for kw in (dict(terms=0), dict(terms=2**31 + 1)):
        ops = [_lib.DotOperand(x.data_ptr(), terms, 1) for x in d]
        r = [C.byref(o) for o in ops]
        o2 = torch.empty((groups, level, 64), dtype=torch.int64, device="cuda:0")
        assert _lib.lib.nflhip_mulrelin_dot_ntt_dev(e.ctx, other.data_ptr(), o2.data_ptr(), r[0], r[1], r[2], r[3], dK.data_ptr(), groups, kw["terms"],
                                                    2, 2, level, 0, None) == _lib.ERR_INVALID


def test_host_variant_equals_device_variant(engine_factory, oracle_factory):
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    groups, terms = 3, 9
    for level in (4, 3):
        ins, Kk, want = case(e, orc, 2, 2, level, terms)
        for plan in PLANS:
            for centered, floor, rescale, square, shared in ((False, False, False, False, False), (True, True, True, False, True),
                                                             (False, False, True, True, False)):
                b = (None, None) if square else tuple(np.array(x[:terms] if shared else x) for x in ins[2:])
                h0, h1 = e.h_mul_relin_dot_ntt(np.array(ins[0]), np.array(ins[1]), b[0], b[1], terms, np.array(Kk), 2, 2, b_shared=shared,
                                               rescale=rescale, centered=centered, floor=floor, plan=plan, level=level)
                w0, w1 = want(centered, floor, rescale, square, shared)
                assert np.array_equal(h0, w0) and np.array_equal(h1, w1), (level, plan, centered, floor, rescale, square, shared)


@pytest.mark.parametrize("plan", ["sequence", "merged"])
def test_two_streams_share_the_scratch(plan, engine_factory, oracle_factory):
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    groups, terms = 3, 9
    ins, Kk, want = case(e, orc, 2, 2, 3, terms)
    ins2, Kk2, want2 = case(e, orc, 2, 2, 3, terms, seed=11)
    d, dK, d2, dK2 = device_operands(e, ins, groups, terms, False), e.to_device(Kk), device_operands(e, ins2, groups, terms, True), e.to_device(Kk2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        r1 = e.mul_relin_dot_ntt(*d, terms, dK, 2, 2, centered=True, plan=plan, stream=s1, level=3)
        r2 = e.mul_relin_dot_ntt(*d2, terms, dK2, 2, 2, b_shared=True, centered=True, plan=plan, stream=s2, level=3)
    torch.cuda.synchronize()
    for got, w in ((r1, want(True, False, False, False, False)), (r2, want2(True, False, False, False, True))):
        assert np.array_equal(e.to_host(got[0]), w[0]) and np.array_equal(e.to_host(got[1]), w[1])


def test_first_call_while_capturing_is_refused_and_the_stream_stays_usable(oracle_factory):
    import torch
    from nfllib_amd import Engine, _lib
    e = Engine(64, 64, 6, device=0)                                               # a context of its own: nothing is warm
    orc = oracle_factory(64, 64, 6)
    try:
        groups, terms, level = 3, 2, 3
        ins, Kk, want = case(e, orc, 2, 2, level, terms)
        w0, w1 = want(False, False, False, False, False)
        d, dK = device_operands(e, ins, groups, terms, False), e.to_device(Kk)
        ops = [_lib.DotOperand(x.data_ptr(), terms, 1) for x in d]
        r = [C.byref(o) for o in ops]
        mr = _lib.lib.nflhip_mulrelin_dot_ntt_dev
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        z = torch.zeros(4, device="cuda:0")
        torch.cuda.synchronize()
        for flags in (_lib.MULRELIN_MERGED, _lib.MULRELIN_SEQUENCE):              # (each plan is cold in its turn)
            o = torch.full((2,) + w0.shape, 5, dtype=torch.int64, device="cuda:0")
            args = (e.ctx, o[0].data_ptr(), o[1].data_ptr(), r[0], r[1], r[2], r[3], dK.data_ptr(), groups, terms, 2, 2, level, flags, sp)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    z.add_(1)
                    rc = mr(*args)
            torch.cuda.synchronize()
            assert rc == _lib.ERR_UNSUPPORTED, (flags, rc)
            assert bool((o == 5).all())                                          # nothing was enqueued
            assert mr(*args) == 0                                                # the same stream
            st.synchronize()
            assert np.array_equal(e.to_host(o[0]), w0) and np.array_equal(e.to_host(o[1]), w1), flags
    finally:
        e.close()


@pytest.mark.parametrize("plan", ["sequence", "merged"])
def test_graph_capture_replays_identically(plan, engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up call, then the same call captured and replayed three times"""
    import torch
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    groups, terms, level = 3, 9, 3
    ins, Kk, want = case(e, orc, 2, 2, level, terms)
    w0, w1 = want(True, False, True, False, False)
    d, dK = device_operands(e, ins, groups, terms, False), e.to_device(Kk)
    both = torch.zeros((2,) + w0.shape, dtype=torch.int64, device="cuda:0")
    out = (both[0], both[1])

    def run():
        e.mul_relin_dot_ntt(*d, terms, dK, 2, 2, rescale=True, centered=True, out=out, plan=plan, level=level)

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        run()                                                  # the warm-up: tables, scratch and child contexts of this many groups
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


def test_real_ciphertexts_decrypt_within_one_key_switch_error(engine_factory, oracle_factory):
    """u64/64/5, K = alpha = 2, a real key, 5 terms: the device's out0 + out1 s is within n dnum alpha 8 2^alpha + n + 1 of the sum of
    the products, decrypted on the host -- the bound of ONE key switch (tests/test_mulrelin_dot_cpu.py)"""
    from test_mulrelin_dot_cpu import phase_error, real_ciphertexts
    lb, n, nm, K, alpha, terms = 64, 64, 5, 2, 2, 5
    L = nm - K
    e, orc, ok = engine_factory(lb, n, nm), oracle_factory(lb, n, nm), oracle_factory(lb, n, L)
    S, key, ops, msg = real_ciphertexts(e.P, K, alpha, n, terms, orc, 1234)
    d = [e.to_device(np.ascontiguousarray(x[0])) for x in ops]
    bound = n * len(key) * alpha * 8 * 2**alpha + n + 1
    for plan in PLANS:
        o0, o1 = e.mul_relin_dot_ntt(*d, terms, e.to_device(key), K, alpha, plan=plan)
        err = phase_error(e.to_host(o0), e.to_host(o1), S, e.P, L, msg, ok)
        print("plan %s: |out0 + out1 s - sum of products|_inf = %d, bound %d" % (plan, err, bound))
        assert 0 < err <= bound, plan


def test_a_chain_across_levels_with_one_key(engine_factory, oracle_factory):
    """the sum of products with the rescale at the top level 4, its result squared at level 3 with the same key"""
    e, orc = engine_factory(64, 64, 6), oracle_factory(64, 64, 6)
    groups, terms = 3, 9
    ins, Kk, want = case(e, orc, 2, 2, 4, terms)
    w = want(False, False, True, False, False)
    w2 = mulrelin_level_rns(w[0], w[1], None, None, Kk, e.P, 2, 2, 3, False, False, True, orc)
    d, dK = device_operands(e, ins, groups, terms, False), e.to_device(Kk)
    c0, c1 = e.mul_relin_dot_ntt(*d, terms, dK, 2, 2, rescale=True)
    assert c0.shape == (groups, 3, 64)
    q0, q1 = e.mul_relin_dot_ntt(c0, c1, None, None, 1, dK, 2, 2, rescale=True, level=3)
    assert np.array_equal(e.to_host(q0), w2[0]) and np.array_equal(e.to_host(q1), w2[1])
    ops = [c0.contiguous(), c1.contiguous()]                                      # and as a sum of one square per group through the strided form
    s0, s1 = e.mul_relin_dot_strided((ops[0], (1, 1)), (ops[1], (1, 1)), None, None, groups, 1, dK, 2, 2, rescale=True, level=3, plan="merged")
    assert np.array_equal(e.to_host(s0), w2[0]) and np.array_equal(e.to_host(s1), w2[1])
