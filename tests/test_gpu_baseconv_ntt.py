"""GPU: the RNS base conversion and the mod-down on NTT-form data (include/nflhip.h "RNS base conversion and mod-down, NTT form",
nfllib_amd/csrc/kernels_baseconv_ntt.hip).  Both plans -- the one-launch kernel and the composed plan -- word for word against
    want = oracle.ntt(baseconv_rns(a))[rows D]        and        want = oracle_kept.ntt(moddown_rns(a))
with the input oracle.ntt(a): the Python-integer restatement of tests/baseconv_util.py between the CPU oracle's transforms.  No
tolerance anywhere.  Shapes: log n = 6 and 7 (both parities of the transforms' first stage), ks on both sides of the 16-term chunk,
moduli past the 92nd, one call on each side of the one-launch kernel's LDS bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from rescale_util import rescale_rns

pytestmark = pytest.mark.gpu

PLANS = ("fused", "composed")
# prefix to suffix, suffix to prefix, middle to all, ks = 1, kd = 1, S = D
PAIRS = {(64, 64, 4): [((0, 2), (2, 2)), ((2, 2), (0, 2)), ((1, 2), (0, 4)), ((3, 1), (0, 4)), ((0, 3), (3, 1)), ((0, 4), (0, 4))],
         (32, 128, 3): [((0, 2), (2, 1)), ((1, 2), (0, 1)), ((1, 1), (0, 3)), ((2, 1), (0, 3)), ((0, 2), (2, 1)), ((0, 3), (0, 3))]}
_INPUTS = {}


def inputs(e, src, seed=3):
    """batch 3, coefficient form: random words; the edge values of rows src planted in polynomial 0, the values around and inside
    the centred band in polynomial 1, every source word p_i - 1 and every y_i = p_i - 1 in the last two positions of polynomial 2"""
    key = (e.limb_bits, e.degree, e.nmoduli, src, seed)
    if key not in _INPUTS:
        P = e.P
        a = B.random_batch(P, e.degree, 3, e.np_dtype, seed)
        n = e.degree                                   # (rows of four words: the values around Q / 2, the band from its lower edge)
        B.plant(a, P, src, B.edge_values(P, src)[-n:], b=0)
        B.plant(a, P, src, B.band_values(P, src, e.limb_bits)[2:][:n] if n < 16 else B.band_values(P, src, e.limb_bits), b=1)
        s = slice(src[0], src[0] + src[1])
        a[2, s, e.degree - 1] = [p - 1 for p in P[s]]
        a[2, s, e.degree - 2] = B.all_y_max(P, src)
        a.setflags(write=False)
        _INPUTS[key] = a
    return _INPUTS[key]


def pattern(e, batch):
    """a recognisable fill for rows that must stay as they are"""
    import torch
    t = torch.arange(batch * e.words_per_poly, dtype=torch.int64, device="cuda:0") % 8191 + 1
    return t.to(e.torch_dtype).reshape(batch, e.nmoduli, e.degree)


def check_pair(e, orc, src, dst, plans=PLANS):
    """both modes, out of place and in place, every plan: rows D equal want, the other rows keep the pattern / the input"""
    import torch
    a = inputs(e, src)
    A = orc.ntt(np.array(a))
    dA = e.to_device(A)
    rows = list(range(dst[0], dst[0] + dst[1]))
    other = [j for j in range(e.nmoduli) if j not in rows]
    for centered in (False, True):
        want = e.to_device(orc.ntt(B.baseconv_rns(a, e.P, src, dst, centered=centered)))
        for plan in plans:
            o = pattern(e, len(a))
            keep = o.clone()
            assert e.baseconv_ntt(dA, src, dst, centered=centered, out=o, plan=plan) is o
            assert torch.equal(o[:, rows], want[:, rows]), (src, dst, centered, plan)
            assert torch.equal(o[:, other], keep[:, other]), (src, dst, centered, plan)
            x = dA.clone()
            assert e.baseconv_ntt(x, src, dst, centered=centered, plan=plan) is x
            assert torch.equal(x[:, rows], want[:, rows]), (src, dst, centered, plan, "in place")
            assert torch.equal(x[:, other], dA[:, other]), (src, dst, centered, plan, "in place")
    assert np.array_equal(e.to_host(dA), A)


def check_down(e, orc, orc_kept, k, seed=6, plans=PLANS):
    """both roundings, every plan, against the restatement; returns the planted input and the expected tensors"""
    import torch
    nm = e.nmoduli
    a = inputs(e, (nm - k, k), seed=seed)
    dA = e.to_device(orc.ntt(np.array(a)))
    out = {}
    for floor in (False, True):
        want = e_kept_device(e, orc_kept.ntt(B.moddown_rns(a, e.P, k, floor=floor)))
        for plan in plans:
            got = e.mod_down_ntt(dA, k, floor=floor, plan=plan)
            assert got.shape == (len(a), nm - k, e.degree) and torch.equal(got, want), (k, floor, plan)
        out[floor] = want
    assert np.array_equal(e.to_host(dA), orc.ntt(np.array(a)))
    return a, out


def e_kept_device(e, arr):
    import torch
    signed = np.ascontiguousarray(arr).view({16: np.int16, 32: np.int32, 64: np.int64}[e.limb_bits])
    return torch.from_numpy(signed.copy()).to("cuda:0")


@pytest.mark.parametrize("lb,n,nm", list(PAIRS))
def test_every_pair_of_ranges_both_plans(lb, n, nm, engine_factory, oracle_factory):
    e, orc = engine_factory(lb, n, nm), oracle_factory(lb, n, nm)
    for src, dst in PAIRS[(lb, n, nm)]:
        check_pair(e, orc, src, dst)
    a = inputs(e, (0, 2))
    up = e.mod_up_ntt(e.to_device(orc.ntt(np.array(a))), (0, 2))
    assert np.array_equal(e.to_host(up), orc.ntt(B.baseconv_rns(a, e.P, (0, 2), (0, nm))))


def test_u16_words_and_a_misaligned_pointer(engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(16, 4, 2), oracle_factory(16, 4, 2), oracle_factory(16, 4, 1)   # rows of 8 bytes: the word variant
    for src, dst in (((0, 1), (1, 1)), ((1, 1), (0, 2)), ((0, 2), (0, 2))):
        check_pair(e, orc, src, dst)
    check_down(e, orc, ok, 1)
    # an output (and an input) one word off 16-byte alignment: the streaming kernel's word variant in the composed mod-down
    e, orc, ok = engine_factory(64, 64, 4), oracle_factory(64, 64, 4), oracle_factory(64, 64, 2)
    a = inputs(e, (2, 2), seed=6)
    A = e.to_device(orc.ntt(np.array(a)))
    buf = torch.zeros(a.size + 1, dtype=torch.int64, device="cuda:0")
    buf[1:].copy_(A.view(-1))
    want = ok.ntt(B.moddown_rns(a, e.P, 2))
    for plan in PLANS:
        for src_ten in (A, buf[1:]):
            out = torch.zeros(3 * 2 * 64 + 1, dtype=torch.int64, device="cuda:0")
            e.mod_down_ntt(src_ten, 2, out=out[1:], plan=plan)
            assert np.array_equal(e.to_host(out[1:]).reshape(3, 2, 64), want) and int(out[0]) == 0, plan
    up = orc.ntt(B.baseconv_rns(a, e.P, (2, 2), (0, 4), centered=True))
    for plan in PLANS:
        buf[1:].copy_(A.view(-1))
        e.baseconv_ntt(buf[1:], (2, 2), (0, 4), centered=True, plan=plan)
        assert np.array_equal(e.to_host(buf[1:]).reshape(a.shape), up) and int(buf[0]) == 0, plan


@pytest.mark.parametrize("src,dst", [((81, 15), (0, 96)), ((70, 17), (60, 36))])
def test_many_rows_mod_up(src, dst, engine_factory, oracle_factory):
    """u64/64/96: ks on both sides of the 16-term chunk, moduli past the 92nd on both sides"""
    e = engine_factory(64, 64, 96)
    assert (2**62 - e.P[92]) >= 2**32 > (2**62 - e.P[91])
    check_pair(e, oracle_factory(64, 64, 96), src, dst)


def test_many_rows_mod_down(engine_factory, oracle_factory):
    check_down(engine_factory(64, 64, 96), oracle_factory(64, 64, 96), oracle_factory(64, 64, 96 - 17), 17)


@pytest.mark.parametrize("lb,nm,k", [(64, 4, 1), (64, 4, 2), (64, 4, 3), (32, 3, 2)])
def test_mod_down_both_plans_floor_and_rounding(lb, nm, k, engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(lb, 64, nm), oracle_factory(lb, 64, nm), oracle_factory(lb, 64, nm - k)
    a, wants = check_down(e, orc, ok, k)
    assert not torch.equal(wants[False], wants[True])                      # the two roundings differ somewhere
    if k == 1:
        b = np.array(a)
        b[:, nm - 1, :][B.in_band(a, e.P, (nm - 1, 1))] = 0                # outside the band: the mod-down by one modulus is the rescale
        dB = e.to_device(orc.ntt(b))
        want = e.rescale(dB, ntt=True)
        assert np.array_equal(e.to_host(want), ok.ntt(rescale_rns(b, e.P)))
        for plan in PLANS:
            assert torch.equal(e.mod_down_ntt(dB, 1, plan=plan), want), plan


def test_the_lds_bound_of_the_one_launch_kernel(engine_factory, oracle_factory):
    """u64/2048/4, rows of 16 KiB: (ks + 1 + centred) rows within 64 KiB (include/nflhip.h)"""
    import torch
    from nfllib_amd import _lib
    e, orc = engine_factory(64, 2048, 4), oracle_factory(64, 2048, 4)
    dst = (0, 4)
    for src, centered, fits in (((0, 2), True, True), ((0, 3), False, True), ((0, 3), True, False), ((0, 4), False, False)):
        assert ((src[1] + 1 + centered) * 2048 * 8 <= 65536) == fits
        a = inputs(e, src)
        dA = e.to_device(orc.ntt(np.array(a)))
        want = e.to_device(orc.ntt(B.baseconv_rns(a, e.P, src, dst, centered=centered)))
        assert torch.equal(e.baseconv_ntt(dA.clone(), src, dst, centered=centered), want), (src, centered)     # the default call
        assert torch.equal(e.baseconv_ntt(dA.clone(), src, dst, centered=centered, plan="composed"), want), (src, centered)
        if fits:
            assert torch.equal(e.baseconv_ntt(dA.clone(), src, dst, centered=centered, plan="fused"), want), (src, centered)
        else:
            with pytest.raises(_lib.NflHipError) as err:
                e.baseconv_ntt(dA.clone(), src, dst, centered=centered, plan="fused")
            assert err.value.code == _lib.ERR_UNSUPPORTED
    # the mod-down: k = 2 rounds (4 rows: fits), k = 3 rounds (5 rows: does not), k = 3 floor (4 rows: fits)
    for k, floor, fits in ((2, False, True), (3, True, True), (3, False, False)):
        a = inputs(e, (4 - k, k), seed=6)
        dA = e.to_device(orc.ntt(np.array(a)))
        want = e_kept_device(e, oracle_factory(64, 2048, 4 - k).ntt(B.moddown_rns(a, e.P, k, floor=floor)))
        assert torch.equal(e.mod_down_ntt(dA, k, floor=floor), want) and torch.equal(e.mod_down_ntt(dA, k, floor=floor, plan="composed"), want)
        if fits:
            assert torch.equal(e.mod_down_ntt(dA, k, floor=floor, plan="fused"), want)
        else:
            with pytest.raises(_lib.NflHipError) as err:
                e.mod_down_ntt(dA, k, floor=floor, plan="fused")
            assert err.value.code == _lib.ERR_UNSUPPORTED


def test_batch_one_equals_polynomial_zero_of_batch_three(engine_factory, oracle_factory):
    import torch
    e, orc = engine_factory(64, 64, 4), oracle_factory(64, 64, 4)
    dA = e.to_device(orc.ntt(np.array(inputs(e, (1, 2)))))
    for plan in PLANS:
        assert torch.equal(e.baseconv_ntt(dA[:1].clone(), (1, 2), (0, 4), centered=True, plan=plan),
                           e.baseconv_ntt(dA.clone(), (1, 2), (0, 4), centered=True, plan=plan)[:1])
        assert torch.equal(e.mod_down_ntt(dA[:1].contiguous(), 2, plan=plan), e.mod_down_ntt(dA, 2, plan=plan)[:1])


@pytest.mark.parametrize("lb,n,nm", [(64, 64, 4), (32, 128, 3), (16, 4, 2)])
def test_compiled_variant_gives_the_same_words(lb, n, nm, engine_factory, compiled_engine_factory):
    import torch
    e, c = engine_factory(lb, n, nm), compiled_engine_factory(lb, n, nm)
    d = e.fill_uniform(e.empty(3), 21, 0)
    k = nm - 1
    for src, dst in (((0, 1), (0, nm)), ((nm - k, k), (0, nm)), ((0, 1), (nm - 1, 1))):
        for centered in (False, True):
            want = e.baseconv_ntt(d.clone(), src, dst, centered=centered)
            for plan in (None,) + PLANS:
                assert torch.equal(c.baseconv_ntt(d.clone(), src, dst, centered=centered, plan=plan), want), (src, dst, centered, plan)
    for floor in (False, True):
        want = e.mod_down_ntt(d, k, floor=floor)
        for plan in (None,) + PLANS:
            assert torch.equal(c.mod_down_ntt(d, k, floor=floor, plan=plan), want)


def test_host_variants_equal_device_variants(engine_factory, oracle_factory):
    e, orc = engine_factory(64, 64, 4), oracle_factory(64, 64, 4)
    a = inputs(e, (1, 2))
    A = orc.ntt(np.array(a))
    for plan in (None,) + PLANS:
        for centered in (False, True):
            assert np.array_equal(e.h_baseconv_ntt(A, (1, 2), (0, 4), centered=centered, plan=plan),
                                  orc.ntt(B.baseconv_rns(a, e.P, (1, 2), (0, 4), centered=centered)))
        got = e.h_baseconv_ntt(A, (3, 1), (0, 1), plan=plan)                 # rows outside D: the input's
        assert np.array_equal(got, orc.ntt(B.baseconv_rns(a, e.P, (3, 1), (0, 1))))
        for floor in (False, True):
            assert np.array_equal(e.h_mod_down_ntt(A, 2, floor=floor, plan=plan), e.to_host(e.mod_down_ntt(e.to_device(A), 2, floor=floor)))


def test_two_streams_share_the_composed_plans_scratch(engine_factory, oracle_factory):
    import torch
    e, orc = engine_factory(64, 64, 4), oracle_factory(64, 64, 4)
    a, b = inputs(e, (0, 2)), inputs(e, (0, 2), seed=11)
    dA, dB = e.to_device(orc.ntt(np.array(a))), e.to_device(orc.ntt(np.array(b)))
    wa = orc.ntt(B.baseconv_rns(a, e.P, (0, 2), (1, 3), centered=True))
    wb = orc.ntt(B.baseconv_rns(b, e.P, (0, 2), (1, 3), centered=True))
    da = oracle_factory(64, 64, 2).ntt(B.moddown_rns(a, e.P, 2))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    xa, xb = dA.clone(), dB.clone()
    torch.cuda.synchronize()
    for _ in range(3):
        e.baseconv_ntt(xa, (0, 2), (1, 3), centered=True, plan="composed", stream=s1)
        e.baseconv_ntt(xb, (0, 2), (1, 3), centered=True, plan="composed", stream=s2)
        ya = e.mod_down_ntt(dA, 2, plan="composed", stream=s1)
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(xa), wa) and np.array_equal(e.to_host(xb), wb) and np.array_equal(e.to_host(ya), da)


def _key_switch_want(e, orc, ok, a, key, src, k):
    """baseconv_ntt -> dot over the batch -> moddown_ntt, on Python integers between the oracle's transforms"""
    U = orc.ntt(B.baseconv_rns(a, e.P, src, (0, e.nmoduli), centered=True)).astype(object)
    D = (U * key.astype(object)).sum(axis=0)
    for j, p in enumerate(e.P):
        D[j] %= p
    d = orc.intt(np.ascontiguousarray(D.astype(e.np_dtype))[None])
    return ok.ntt(B.moddown_rns(d, e.P, k))


@pytest.mark.parametrize("plan", PLANS)
def test_graph_capture_replays_identically(plan, engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up of the same calls, then baseconv_ntt + dot + moddown_ntt captured"""
    import torch
    e, orc, ok = engine_factory(64, 64, 4), oracle_factory(64, 64, 4), oracle_factory(64, 64, 2)
    src, k = (0, 2), 2
    a = inputs(e, src)
    key = B.random_batch(e.P, 64, 3, e.np_dtype, 17)
    want = _key_switch_want(e, orc, ok, a, key, src, k)
    dA, dK = e.to_device(orc.ntt(np.array(a))), e.to_device(key)
    u, d = torch.zeros_like(dA), torch.zeros_like(dA[:1])
    y = torch.zeros((1, 2, 64), dtype=torch.int64, device="cuda:0")

    def run():
        e.baseconv_ntt(dA, src, (0, 4), centered=True, out=u, plan=plan)
        e.dot(u, dK, 3, out=d)
        e.mod_down_ntt(d, k, out=y, plan=plan)

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        run()                                                  # the warm-up: tables, scratch and child contexts of this batch
        st.synchronize()
        assert np.array_equal(e.to_host(y), want)
        with torch.cuda.graph(g, stream=st):
            run()
    for _ in range(3):
        u.zero_(), d.zero_(), y.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(e.to_host(y), want)


def test_first_call_while_capturing_is_refused_and_the_stream_stays_usable(oracle_factory):
    import torch
    from nfllib_amd import Engine, _lib
    e, orc = Engine(64, 64, 4, device=0), oracle_factory(64, 64, 4)      # a context of its own: nothing is warm
    try:
        a = inputs(e, (0, 2))
        dA = e.to_device(orc.ntt(np.array(a)))
        want = orc.ntt(B.baseconv_rns(a, e.P, (0, 2), (0, 4)))
        x, z = dA.clone(), torch.zeros(4, device="cuda:0")
        st = torch.cuda.Stream()
        bc = _lib.lib.nflhip_baseconv_ntt_dev
        sp = C.c_void_p(st.cuda_stream)
        rcs = []
        torch.cuda.synchronize()
        for flags, warm in ((_lib.BASECONV_NTT_FUSED, None), (_lib.BASECONV_NTT_COMPOSED, "fused")):
            if warm:                                           # the tables are there; the composed plan's scratch and children are not
                e.baseconv_ntt(dA.clone(), (0, 2), (0, 4), plan=warm, stream=st)
                st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    z.add_(1)
                    rcs.append(bc(e.ctx, x.data_ptr(), x.data_ptr(), 3, 0, 2, 0, 4, flags, sp))
            torch.cuda.synchronize()
            assert rcs[-1] == _lib.ERR_UNSUPPORTED, rcs
            assert np.array_equal(e.to_host(x), e.to_host(dA))      # nothing was enqueued
            y = dA.clone()
            torch.cuda.synchronize()
            assert bc(e.ctx, y.data_ptr(), y.data_ptr(), 3, 0, 2, 0, 4, flags, sp) == 0     # the same stream, after the capture
            st.synchronize()
            assert np.array_equal(e.to_host(y), want)
    finally:
        e.close()


def test_identities_through_the_engines_own_entries(engine_factory):
    import torch
    e = engine_factory(64, 64, 4)
    x = e.to_device(inputs(e, (1, 2)))
    for plan in PLANS:
        for centered in (False, True):
            got = e.intt_(e.baseconv_ntt(e.ntt_(x.clone()), (1, 2), (0, 4), centered=centered, plan=plan))
            assert torch.equal(got, e.baseconv(x.clone(), (1, 2), (0, 4), centered=centered)), (plan, centered)
    x = e.to_device(inputs(e, (2, 2), seed=6))
    kept = engine_factory(64, 64, 2)
    for plan in PLANS:
        for floor in (False, True):
            got = kept.intt_(e.mod_down_ntt(e.ntt_(x.clone()), 2, floor=floor, plan=plan))
            assert torch.equal(got, e.mod_down(x, 2, floor=floor)), (plan, floor)


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    L, ERR = _lib.lib, _lib.ERR_INVALID
    N = 64
    e = engine_factory(64, N, 4)
    d = e.fill_uniform(e.empty(4), 1, 0)
    o = torch.zeros((8, 4, N), dtype=torch.int64, device="cuda:0")
    p, q = d.data_ptr(), o.data_ptr()
    row = N * 8
    bc, md = L.nflhip_baseconv_ntt_dev, L.nflhip_moddown_ntt_dev
    assert bc(None, q, p, 4, 0, 2, 2, 2, 0, None) == ERR                       # NULL context
    assert bc(e.ctx, None, p, 4, 0, 2, 2, 2, 0, None) == ERR                   # NULL output
    assert bc(e.ctx, q, None, 4, 0, 2, 2, 2, 0, None) == ERR                   # NULL input
    for s0, ks, d0, kd in ((0, 0, 0, 1), (0, 1, 0, 0), (4, 1, 0, 1), (3, 2, 0, 1), (0, 5, 0, 1), (0, 1, 4, 1), (0, 1, 2, 3),
                           (0, 2**63, 0, 1), (2**64 - 1, 2, 0, 1), (0, 1, 2**64 - 1, 2)):
        assert bc(e.ctx, q, p, 4, s0, ks, d0, kd, 0, None) == ERR, (s0, ks, d0, kd)   # ranges
    for flags in (0x600, 0x700, 1, 2, 0x800, 0x201, 0x402, -1):                # both plan flags; unknown bits
        assert bc(e.ctx, q, p, 4, 0, 2, 2, 2, flags, None) == ERR, flags
        assert md(e.ctx, q, p, 4, 1, flags, None) == ERR, flags
    assert bc(e.ctx, p + row, p, 4, 0, 2, 2, 2, 0, None) == ERR                # an overlap that is not "the same buffer"
    assert bc(e.ctx, p - 16 * row + 8, p, 4, 0, 2, 2, 2, 0, None) == ERR       # output's last word on the input's first
    assert bc(e.ctx, q, p, 2**61, 0, 2, 2, 2, 0, None) == ERR                  # the size overflows
    for k in (0, 4, 5, 2**64 - 1):
        assert md(e.ctx, q, p, 4, k, 0, None) == ERR                           # k out of range
    assert md(e.ctx, p, p, 4, 1, 0, None) == ERR                               # mod-down in place
    assert md(e.ctx, p + row, p, 4, 1, 0, None) == ERR                         # output inside the input
    assert md(e.ctx, p - 12 * row + 8, p, 4, 1, 0, None) == ERR                # output's last word on the input's first
    assert md(e.ctx, None, p, 4, 1, 0, None) == ERR and md(e.ctx, q, None, 4, 1, 0, None) == ERR
    assert md(None, q, p, 4, 1, 0, None) == ERR
    h = e.to_host(d)
    ho = np.zeros_like(h)
    hp = h.ctypes.data
    assert L.nflhip_baseconv_ntt(e.ctx, ho.ctypes.data, hp, 4, 0, 2, 2, 3, 0) == ERR    # host: ranges
    assert L.nflhip_baseconv_ntt(e.ctx, None, hp, 4, 0, 2, 2, 2, 0) == ERR              # host: NULL
    assert L.nflhip_baseconv_ntt(e.ctx, hp + row, hp, 2, 0, 2, 2, 2, 0) == ERR          # host: overlap
    assert L.nflhip_baseconv_ntt(e.ctx, ho.ctypes.data, hp, 4, 0, 2, 2, 2, 0x600) == ERR  # host: both plan flags
    assert L.nflhip_moddown_ntt(e.ctx, hp, hp, 4, 1, 0) == ERR                          # host: in place
    assert L.nflhip_moddown_ntt(e.ctx, ho.ctypes.data, hp, 4, 4, 0) == ERR              # host: k
    for flags in (0, 0x200, 0x400):
        assert bc(e.ctx, None, None, 0, 0, 2, 2, 2, flags, None) == 0              # an empty batch is fine
        assert md(e.ctx, None, None, 0, 1, flags, None) == 0
    # a repeated source modulus is refused by the table builder, on the host: a context over moduli 0, 1, 0
    from nfllib_amd.params import params
    pr = params(64)
    idx = [0, 1, 0]
    tabs = [np.ascontiguousarray(t[idx]) for t in (pr.P, pr.primitive_roots, pr.invkmax)]
    ctx = C.c_void_p()
    assert L.nflhip_ctx_create(C.byref(ctx), 0, 64, N, 3, *[t.ctypes.data_as(C.c_void_p) for t in tabs], pr.kmax_log2) == 0
    try:
        for flags in (0, 0x200, 0x400):
            assert bc(ctx, q, p, 1, 0, 3, 0, 3, flags, None) == ERR
            assert b"source modulus repeats" in L.nflhip_last_error(ctx)
            assert md(ctx, q, p, 1, 1, flags, None) == ERR                          # the kept row 0 repeats the dropped modulus
        assert bc(ctx, q, p, 1, 0, 2, 2, 1, 0, None) == 0                           # distinct sources: served
    finally:
        torch.cuda.synchronize()
        L.nflhip_ctx_destroy(ctx)
    # nothing refused above wrote anything, and the context still works
    torch.cuda.synchronize()
    assert np.array_equal(e.to_host(d), h)
    o.zero_()
    assert bc(e.ctx, q, p, 4, 0, 2, 2, 2, 0, None) == 0
    torch.cuda.synchronize()
    assert not o[:4, :2].any() and not o[4:].any() and o[:4, 2:].any()


@pytest.fixture(scope="module")
def cpp_program(tmp_path_factory):
    from test_baseconv_ntt_cpu import build_cpp
    return build_cpp(str(tmp_path_factory.mktemp("cpp_baseconv_ntt")), gpu=True)


@pytest.mark.parametrize("devs,batch", [("0,0,0", 5), ("0,0,0,0", 3), ("0", 4)])
def test_cpp_surface_on_the_gpu(cpp_program, devs, batch):
    """the program of tests/cpp_baseconv_ntt against the real library: poly, poly_p, device_batch and a sharded_batch of several
    shards on device 0 (a batch that does not divide, empty shards), and the identities through the transforms"""
    r = subprocess.run([cpp_program, devs, str(batch), "real"], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
