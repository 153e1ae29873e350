"""GPU: the scale-invariant tensor product of BFV and the multiplication with relinearisation built on it (include/nflhip.h "BFV
multiplication").  nflhip_bfv_tensor_ntt_dev against the four steps of its definition through the existing entries and
nflhip_scale_round_ntt_dev, and against the Python-integer restatement between the CPU oracle's transforms; then real ciphertexts:
Engine.bfv_mul_relin_ntt with a key from tests/mulrelin_util.py relin_key decrypts on the host to m1 m2 mod t.  No tolerance."""
import numpy as np
import pytest

import baseconv_util as B
import scale_round_util as S
from mulrelin_util import relin_key, tensor_rns

pytestmark = pytest.mark.gpu

N, L, KB, BATCH = 64, 2, 3, 2
SHAPES = [(32, 257), (64, 65537)]
_CACHE = {}


def case(e, orc, ol, t):
    """four NTT-form inputs over the first L moduli and, computed on demand and kept, the restatement of (floor, square)"""
    key = (e.limb_bits, t)
    if key not in _CACHE:
        ins = [B.random_batch(e.P[:L], N, BATCH, e.np_dtype, 70 + k) for k in range(4)]
        for x in ins:
            x.setflags(write=False)
        _CACHE[key] = (ins, {})
    ins, wants = _CACHE[key]

    def want(floor=False, square=False):
        if (floor, square) not in wants:
            ext = []
            for x in (ins[:2] if square else ins):
                X = np.zeros((BATCH, e.nmoduli, N), dtype=e.np_dtype)
                X[:, :L] = ol.intt(np.array(x))
                ext.append(orc.ntt(B.baseconv_rns(X, e.P, (0, L), (0, e.nmoduli), centered=True)))
            d = tensor_rns(ext[0], ext[1], None if square else ext[2], None if square else ext[3], e.P)
            wants[(floor, square)] = [ol.ntt(S.scale_round_rns(orc.intt(np.ascontiguousarray(c)), e.P, L, t, floor=floor)) for c in d]
        return wants[(floor, square)]
    return ins, want


@pytest.mark.parametrize("lb,t", SHAPES)
def test_tensor_equals_its_definition_and_the_restatement(lb, t, engine_factory, oracle_factory):
    import torch
    nm = L + KB
    e, orc, ol = engine_factory(lb, N, nm), oracle_factory(lb, N, nm), oracle_factory(lb, N, L)
    ins, want = case(e, orc, ol, t)
    d = [e.to_device(x) for x in ins]
    for floor in (False, True):
        for square in (False, True):
            b = (None, None) if square else (d[2], d[3])
            got = e.bfv_tensor_ntt(d[0], d[1], b[0], b[1], L, t, floor=floor)
            assert all(g.shape == (BATCH, L, N) for g in got)
            # the four steps through the existing entries
            ext = []
            for x in (d[:2] if square else d):
                E = torch.zeros((BATCH, nm, N), dtype=e.torch_dtype, device="cuda:0")
                E[:, :L] = x
                ext.append(e.baseconv_ntt(E, (0, L), (0, nm), centered=True))
            ten = e.tensor_ntt(ext[0], ext[1], None if square else ext[2], None if square else ext[3])
            for g, c, w in zip(got, ten, want(floor, square)):
                assert torch.equal(g, e.scale_round(c.contiguous(), L, t, floor=floor, ntt=True)), (floor, square)
                assert np.array_equal(e.to_host(g), w), (floor, square)
            # the forced two-pass plan, and outputs that do not follow each other in memory, one of them an input
            two = e.bfv_tensor_ntt(d[0], d[1], b[0], b[1], L, t, floor=floor, plan="two_pass")
            alias = d[1].clone()
            outs = (torch.zeros_like(d[0]), alias, torch.zeros_like(d[0]))
            e.bfv_tensor_ntt(d[0], alias, b[0], b[1], L, t, floor=floor, outs=outs)
            for g, x, y in zip(got, two, outs):
                assert torch.equal(g, x) and torch.equal(g, y), (floor, square)
    hw = e.h_bfv_tensor_ntt(ins[0], ins[1], ins[2], ins[3], L, t)
    assert all(np.array_equal(x, y) for x, y in zip(hw, want()))
    for x, h in zip(d, ins):
        assert np.array_equal(e.to_host(x), h)


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    ERR, fn = _lib.ERR_INVALID, _lib.lib.nflhip_bfv_tensor_ntt_dev
    e = engine_factory(64, N, L + KB)
    x = [torch.zeros((BATCH, L, N), dtype=torch.int64, device="cuda:0") for _ in range(7)]
    p = [v.data_ptr() for v in x]
    assert fn(e.ctx, p[0], p[1], p[2], p[3], p[4], p[5], p[6], BATCH, L, 65537, 0, None) == 0
    assert fn(None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], BATCH, L, 65537, 0, None) == ERR
    for ks in (0, L + KB):
        assert fn(e.ctx, p[0], p[1], p[2], p[3], p[4], p[5], p[6], BATCH, ks, 65537, 0, None) == ERR
    for t in (0, 2**61):
        assert fn(e.ctx, p[0], p[1], p[2], p[3], p[4], p[5], p[6], BATCH, L, t, 0, None) == ERR
    for flags in (1, _lib.SCALE_ROUND_KEEP, 0x800):
        assert fn(e.ctx, p[0], p[1], p[2], p[3], p[4], p[5], p[6], BATCH, L, 65537, flags, None) == ERR     # KEEP is not a flag of the product
    assert fn(e.ctx, p[0], p[1], p[2], p[3], p[4], p[5], None, BATCH, L, 65537, 0, None) == ERR            # one of b0, b1 NULL
    assert fn(e.ctx, p[0], p[0], p[2], p[3], p[4], p[5], p[6], BATCH, L, 65537, 0, None) == ERR            # two outputs overlap
    assert fn(e.ctx, p[3] + 8, p[1], p[2], p[3], p[4], p[5], p[6], BATCH, L, 65537, 0, None) == ERR        # an output inside an input
    assert fn(e.ctx, None, None, None, None, None, None, None, 0, L, 65537, 0, None) == 0                 # an empty batch


@pytest.mark.parametrize("lb,t", SHAPES)
def test_product_with_relinearisation_decrypts(lb, t, engine_factory, oracle_factory):
    """K = 1 special modulus, alpha = 1: fresh encryptions of m1, m2 (ternary secret, noise in [-3, 3]) -> bfv_mul_relin_ntt ->
    round(t (out0 + out1 s) / Q) mod t = m1 m2 mod t in Z_t[x] / (x^n + 1), the product and the square"""
    K, alpha, nm = 1, 1, L + KB
    e, eks = engine_factory(lb, N, nm), engine_factory(lb, N, L + K)
    oks, ol = oracle_factory(lb, N, L + K), oracle_factory(lb, N, L)
    P = e.P
    Q, Bp = B.prod(P[:L]), B.prod(P[L:])
    assert N * Q * Q // 2 < Q * Bp // 2 and t * N * Q // 2 + 1 < Bp // 2          # the caller's bound (include/nflhip.h)
    rnd = np.random.RandomState(5)
    s = S.bfv_keygen(N, rnd)
    Pk = P[:L + K]
    Sn = oks.ntt(B.rows_of(np.array(s, dtype=object), Pk, range(L + K), e.np_dtype)[None])[0].astype(object)
    S2 = np.empty_like(Sn)
    for j, p in enumerate(Pk):
        S2[j] = Sn[j] * Sn[j] % p
    key = relin_key(Pk, K, alpha, N, Sn, S2, oks, rnd, dtype=e.np_dtype)
    msgs = [[[int(x) for x in rnd.randint(0, t, size=N)] for _ in range(BATCH)] for _ in range(2)]
    cts = [[S.bfv_encrypt(m, s, Q, t, rnd) for m in ms] for ms in msgs]

    def comp(side, c):                                                           # component c of every ciphertext of a side, NTT form
        rows = np.concatenate([S.lists_to_rows(ct[c], P[:L], e.np_dtype) for ct in cts[side]])
        return e.to_device(ol.ntt(rows))
    a0, a1, b0, b1 = comp(0, 0), comp(0, 1), comp(1, 0), comp(1, 1)
    dk = eks.to_device(key)
    for bb, other in (((b0, b1), 1), ((None, None), 0)):
        o0, o1 = e.bfv_mul_relin_ntt(eks, a0, a1, bb[0], bb[1], dk, L, t, K, alpha)
        c0, c1 = ol.intt(e.to_host(o0)), ol.intt(e.to_host(o1))
        for k in range(BATCH):
            got = S.bfv_decrypt((S.rows_to_list(c0[k], P[:L]), S.rows_to_list(c1[k], P[:L])), s, Q, t)
            assert got == [x % t for x in S.negacyclic(msgs[0][k], msgs[other][k])], (lb, k, other)
