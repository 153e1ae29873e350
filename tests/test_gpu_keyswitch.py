"""GPU: the hybrid key switch in NTT form (include/nflhip.h "hybrid key switching", nfllib_amd/csrc/kernels_keyswitch.hip).  Every plan
-- the sequence of existing entries, the composed plan with its all-digit mod-up kernel, the one-launch kernel -- both mod-up modes and
both roundings, word for word against tests/keyswitch_util.py keyswitch_rns: the header's definition on Python integers between the
CPU oracle's transforms.  No tolerance anywhere.  Inputs are oracle.ntt of batches of 3 with, per digit, the edge values, the values
around and inside the centred band and every y_i = p_i - 1 planted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import baseconv_util as B
from keyswitch_util import digits, keyswitch_rns

pytestmark = pytest.mark.gpu

PLANS = ("sequence", "composed", "fused")
MODES = [(c, f) for c in (False, True) for f in (False, True)]
_CACHE = {}


def planted(e, K, alpha, seed=3):
    """coefficient form, [3, L, n]: random words; per digit the edge values in polynomial 0, the band values in polynomial 1, every
    source word p_i - 1 and every y_i = p_i - 1 in polynomial 2 -- each digit in positions of its own"""
    nm, n = e.nmoduli, e.degree
    S = digits(nm, K, alpha)
    a = B.random_batch(e.P[:nm - K], n, 3, e.np_dtype, seed)
    width = max(1, n // len(S))
    for d, src in enumerate(S):
        first = (d * width) % n
        B.plant(a, e.P, src, B.edge_values(e.P, src)[-width:], b=0, first=first)
        B.plant(a, e.P, src, B.band_values(e.P, src, e.limb_bits)[2:][:width], b=1, first=first)
        s = slice(src[0], src[0] + src[1])
        a[2, s, first] = B.all_y_max(e.P, src)
        if width > 1:
            a[2, s, first + 1] = [p - 1 for p in e.P[s]]
    return a


def case(e, orc, ok, K, alpha, seed=3):
    """the NTT-form input, the key and, computed on demand and kept, the expected outputs of a mode"""
    key = (e.limb_bits, e.degree, e.nmoduli, K, alpha, seed)
    if key not in _CACHE:
        dnum = len(digits(e.nmoduli, K, alpha))
        A = ok.ntt(planted(e, K, alpha, seed))
        Kk = B.random_batch(e.P, e.degree, 2 * dnum, e.np_dtype, seed + 100).reshape(dnum, 2, e.nmoduli, e.degree)
        A.setflags(write=False), Kk.setflags(write=False)
        _CACHE[key] = (A, Kk, {})
    A, Kk, wants = _CACHE[key]

    def want(centered, floor):
        if (centered, floor) not in wants:
            wants[(centered, floor)] = keyswitch_rns(A, Kk, e.P, K, alpha, centered, floor, orc, ok)
        return wants[(centered, floor)]
    return A, Kk, want


def check(e, orc, ok, K, alpha, plans=PLANS, modes=MODES):
    import torch
    A, Kk, want = case(e, orc, ok, K, alpha)
    dA, dK = e.to_device(A), e.to_device(Kk)
    assert e.keyswitch_digits(K, alpha) == len(Kk)
    for centered, floor in modes:
        w0, w1 = (e.to_device(w) for w in want(centered, floor))
        for plan in plans:
            o0, o1 = e.key_switch_ntt(dA, dK, K, alpha, centered=centered, floor=floor, plan=plan)
            assert o0.shape == o1.shape == dA.shape
            assert torch.equal(o0, w0) and torch.equal(o1, w1), (K, alpha, centered, floor, plan)
    assert np.array_equal(e.to_host(dA), A) and np.array_equal(e.to_host(dK), Kk)


@pytest.mark.parametrize("lb,n,nm,K,alpha", [(64, 64, 5, 2, 1), (64, 64, 5, 2, 2), (64, 64, 5, 2, 3), (64, 128, 5, 1, 3), (32, 128, 4, 1, 2),
                                             (16, 4, 2, 1, 1), (64, 64, 20, 2, 1)])
def test_every_plan_both_modes_both_roundings(lb, n, nm, K, alpha, engine_factory, oracle_factory):
    """dnum 3, 2 with a short last digit, 1; the other parity of log n; 32- and 16-bit limbs (rows of 8 bytes: the word variants;
    the parameter set has two 16-bit moduli, so u16/4/2 with K = alpha = 1 is the one 16-bit key switch there is); 18 digits, across
    the 16-term accumulate chunk"""
    check(engine_factory(lb, n, nm), oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K), K, alpha)
    check(engine_factory(lb, n, nm), oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K), K, alpha, plans=(None,), modes=MODES[:1])


def test_many_rows_digits_past_the_chunk_and_moduli_past_the_92nd(engine_factory, oracle_factory):
    """u64/64/96, K = alpha = 17: L = 79, five digits, the last of 11 rows: ks crosses the 16-row chunk, moduli past the 92nd among
    sources and destinations.  By the stated bound the one-launch kernel FITS here -- (79 + 1) rows of 512 bytes are 40 KiB, plus
    640 bytes of corrections when centred -- so it is checked like the other plans; a forced call past the bound is refused in
    test_the_lds_bound_of_the_one_launch_kernel."""
    e, orc, ok = engine_factory(64, 64, 96), oracle_factory(64, 64, 96), oracle_factory(64, 64, 79)
    assert (2**62 - e.P[92]) >= 2**32 > (2**62 - e.P[91]) and e.keyswitch_digits(17, 17) == 5
    assert (79 + 1) * 64 * 8 + 2 * 5 * 64 <= 65536
    check(e, orc, ok, 17, 17, plans=PLANS + (None,), modes=[(False, False), (True, True)])


def test_every_buffer_one_word_off_alignment_with_guard_words(engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    A, Kk, want = case(e, orc, ok, 2, 2)
    w0, w1 = want(True, False)
    a = torch.zeros(A.size + 2, dtype=torch.int64, device="cuda:0")
    k = torch.zeros(Kk.size + 2, dtype=torch.int64, device="cuda:0")
    a[1:-1].copy_(e.to_device(A).view(-1)), k[1:-1].copy_(e.to_device(Kk).view(-1))
    for plan in PLANS:
        o0, o1 = (torch.full((A.size + 2,), 7, dtype=torch.int64, device="cuda:0") for _ in range(2))
        e.key_switch_ntt(a[1:-1], k[1:-1], 2, 2, centered=True, out=(o0[1:-1], o1[1:-1]), plan=plan)
        for o, w in ((o0, w0), (o1, w1)):
            assert np.array_equal(e.to_host(o[1:-1]).reshape(w.shape), w) and int(o[0]) == 7 and int(o[-1]) == 7, plan
    assert int(a[0]) == 0 and int(a[-1]) == 0 and int(k[0]) == 0 and int(k[-1]) == 0


def test_the_lds_bound_of_the_one_launch_kernel(engine_factory, oracle_factory):
    """(L + 1) n sizeof(T) + [centred] 2 dnum n <= 64 KiB: u64/2048 with L = 3 fits in fast mode only, L = 4 does not fit, L = 2 fits
    centred as well"""
    import torch
    from nfllib_amd import _lib
    for nm, centered, fits in ((4, False, True), (4, True, False), (5, False, False), (3, True, True)):
        L = nm - 1
        assert ((L + 1) * 2048 * 8 + (2 * L * 2048 if centered else 0) <= 65536) == fits
        e, orc, ok = engine_factory(64, 2048, nm), oracle_factory(64, 2048, nm), oracle_factory(64, 2048, L)
        A, Kk, want = case(e, orc, ok, 1, 1)
        dA, dK = e.to_device(A), e.to_device(Kk)
        w = [e.to_device(x) for x in want(centered, False)]
        for plan in (None, "composed") + (("fused",) if fits else ()):
            got = e.key_switch_ntt(dA, dK, 1, 1, centered=centered, plan=plan)
            assert torch.equal(got[0], w[0]) and torch.equal(got[1], w[1]), (nm, centered, plan)
        if not fits:
            with pytest.raises(_lib.NflHipError) as err:
                e.key_switch_ntt(dA, dK, 1, 1, centered=centered, plan="fused")
            assert err.value.code == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()


def test_batch_one_equals_polynomial_zero_of_batch_three(engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    A, Kk, _ = case(e, orc, ok, 2, 2)
    dA, dK = e.to_device(A), e.to_device(Kk)
    for plan in PLANS:
        one, three = e.key_switch_ntt(dA[:1].contiguous(), dK, 2, 2, plan=plan), e.key_switch_ntt(dA, dK, 2, 2, plan=plan)
        assert torch.equal(one[0], three[0][:1]) and torch.equal(one[1], three[1][:1]), plan


@pytest.mark.parametrize("lb,n,nm,K,alpha", [(64, 64, 5, 2, 2), (32, 128, 4, 1, 2), (16, 4, 2, 1, 1)])
def test_compiled_variant_gives_the_same_words(lb, n, nm, K, alpha, engine_factory, compiled_engine_factory, oracle_factory):
    import torch
    e, c = engine_factory(lb, n, nm), compiled_engine_factory(lb, n, nm)
    A, Kk, want = case(e, oracle_factory(lb, n, nm), oracle_factory(lb, n, nm - K), K, alpha)
    dA, dK = e.to_device(A), e.to_device(Kk)
    for centered, floor in ((False, False), (True, True)):
        w = [e.to_device(x) for x in want(centered, floor)]
        for plan in (None,) + PLANS:
            got = c.key_switch_ntt(dA, dK, K, alpha, centered=centered, floor=floor, plan=plan)
            assert torch.equal(got[0], w[0]) and torch.equal(got[1], w[1]), (centered, floor, plan)


def test_host_variant_equals_device_variant(engine_factory, oracle_factory):
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    A, Kk, want = case(e, orc, ok, 2, 2)
    for plan in (None,) + PLANS:
        for centered, floor in ((False, False), (True, True)):
            h0, h1 = e.h_key_switch_ntt(np.array(A), np.array(Kk), 2, 2, centered=centered, floor=floor, plan=plan)
            d0, d1 = e.key_switch_ntt(e.to_device(A), e.to_device(Kk), 2, 2, centered=centered, floor=floor, plan=plan)
            w0, w1 = want(centered, floor)
            assert np.array_equal(h0, w0) and np.array_equal(h1, w1), (plan, centered, floor)
            assert np.array_equal(e.to_host(d0), h0) and np.array_equal(e.to_host(d1), h1)


@pytest.mark.parametrize("plan", PLANS)
def test_two_streams_share_the_scratch(plan, engine_factory, oracle_factory):
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    A, Kk, want = case(e, orc, ok, 2, 1)
    A2, Kk2, want2 = case(e, orc, ok, 2, 1, seed=11)
    dA, dK, dA2, dK2 = (e.to_device(x) for x in (A, Kk, A2, Kk2))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        r1 = e.key_switch_ntt(dA, dK, 2, 1, centered=True, plan=plan, stream=s1)
        r2 = e.key_switch_ntt(dA2, dK2, 2, 1, centered=True, plan=plan, stream=s2)
    torch.cuda.synchronize()
    for got, w in ((r1, want(True, False)), (r2, want2(True, False))):
        assert np.array_equal(e.to_host(got[0]), w[0]) and np.array_equal(e.to_host(got[1]), w[1])


@pytest.mark.parametrize("plan", PLANS)
def test_graph_capture_replays_identically(plan, engine_factory, oracle_factory):
    """one stream, no parallel branches: a warm-up call, then the same call captured and replayed three times"""
    import torch
    e, orc, ok = engine_factory(64, 64, 5), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)
    A, Kk, want = case(e, orc, ok, 2, 2)
    w0, w1 = want(True, False)
    dA, dK = e.to_device(A), e.to_device(Kk)
    both = torch.zeros((2,) + A.shape, dtype=torch.int64, device="cuda:0")
    out = (both[0], both[1])

    def run():
        e.key_switch_ntt(dA, dK, 2, 2, centered=True, out=out, plan=plan)

    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        run()                                                  # the warm-up: tables, scratch and child contexts of this batch
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
    e, orc, ok = Engine(64, 64, 5, device=0), oracle_factory(64, 64, 5), oracle_factory(64, 64, 3)   # a context of its own: nothing is warm
    try:
        A, Kk, want = case(e, orc, ok, 2, 2)
        w0, w1 = want(False, False)
        dA, dK = e.to_device(A), e.to_device(Kk)
        ks = _lib.lib.nflhip_keyswitch_ntt_dev
        st = torch.cuda.Stream()
        sp = C.c_void_p(st.cuda_stream)
        z = torch.zeros(4, device="cuda:0")
        torch.cuda.synchronize()
        for flags in (_lib.KEYSWITCH_FUSED, _lib.KEYSWITCH_COMPOSED, _lib.KEYSWITCH_SEQUENCE):   # (each plan is cold in its turn)
            o = torch.full((2,) + A.shape, 5, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    z.add_(1)
                    rc = ks(e.ctx, o[0].data_ptr(), o[1].data_ptr(), dA.data_ptr(), dK.data_ptr(), 3, 2, 2, flags, sp)
            torch.cuda.synchronize()
            assert rc == _lib.ERR_UNSUPPORTED, (flags, rc)
            assert bool((o == 5).all())                                  # nothing was enqueued
            assert ks(e.ctx, o[0].data_ptr(), o[1].data_ptr(), dA.data_ptr(), dK.data_ptr(), 3, 2, 2, flags, sp) == 0   # the same stream
            st.synchronize()
            assert np.array_equal(e.to_host(o[0]), w0) and np.array_equal(e.to_host(o[1]), w1), flags
    finally:
        e.close()


def test_invalid_arguments(engine_factory):
    import torch
    from nfllib_amd import _lib
    from nfllib_amd.params import params
    Lb, ERR = _lib.lib, _lib.ERR_INVALID
    N, nm, K, alpha = 64, 5, 2, 2
    e = engine_factory(64, N, nm)
    row, batch, L, dnum = N * 8, 2, nm - K, 2
    a = torch.ones((batch, L, N), dtype=torch.int64, device="cuda:0")
    k = torch.ones((dnum, 2, nm, N), dtype=torch.int64, device="cuda:0")
    o = torch.full((2, batch, L, N), 9, dtype=torch.int64, device="cuda:0")
    pa, pk, p0, p1 = a.data_ptr(), k.data_ptr(), o[0].data_ptr(), o[1].data_ptr()
    ks, hk = Lb.nflhip_keyswitch_ntt_dev, Lb.nflhip_keyswitch_ntt
    assert ks(None, p0, p1, pa, pk, batch, K, alpha, 0, None) == ERR                       # NULL context
    for args in ((None, p1, pa, pk), (p0, None, pa, pk), (p0, p1, None, pk), (p0, p1, pa, None)):
        assert ks(e.ctx, *args, batch, K, alpha, 0, None) == ERR                          # a NULL pointer
    for kk in (0, nm, nm + 1, 2**64 - 1):
        assert ks(e.ctx, p0, p1, pa, pk, batch, kk, 1, 0, None) == ERR, kk                 # k_special out of range
        assert Lb.nflhip_keyswitch_digits(e.ctx, kk, 1) == 0
    for al in (0, L + 1, 2**64 - 1):
        assert ks(e.ctx, p0, p1, pa, pk, batch, K, al, 0, None) == ERR, al                 # alpha out of range
        assert Lb.nflhip_keyswitch_digits(e.ctx, K, al) == 0
    assert Lb.nflhip_keyswitch_digits(None, K, alpha) == 0
    assert [Lb.nflhip_keyswitch_digits(e.ctx, K, al) for al in (1, 2, 3)] == [3, 2, 1]
    for flags in (1, 2, 0x80, 0x2000, -1, 0xC00, 0x1400, 0x1800, 0x1C00):                  # unknown bits; two plan flags
        assert ks(e.ctx, p0, p1, pa, pk, batch, K, alpha, flags, None) == ERR, flags
    assert ks(e.ctx, p0, p1, pa, pk, 2**61, K, alpha, 0, None) == ERR                      # the size overflows
    ob = batch * L * row
    for args in ((p0, p0, pa, pk), (p0, p0 + ob - 8, pa, pk), (pa, p1, pa, pk), (p0, pa + 8, pa, pk), (pk, p1, pa, pk),
                 (p0, pk + 2 * dnum * nm * row - 8, pa, pk), (p0, p1, pk + row, pk), (p0, p1, pa, pa - 2 * dnum * nm * row + 8)):
        assert ks(e.ctx, *args, batch, K, alpha, 0, None) == ERR, args                    # every pair overlapping
    ha, hk_, h0, h1 = e.to_host(a), e.to_host(k), np.zeros((batch, L, N), np.uint64), np.zeros((batch, L, N), np.uint64)
    assert hk(e.ctx, h0.ctypes.data, h0.ctypes.data, ha.ctypes.data, hk_.ctypes.data, batch, K, alpha, 0) == ERR     # host: overlap
    assert hk(e.ctx, h0.ctypes.data, None, ha.ctypes.data, hk_.ctypes.data, batch, K, alpha, 0) == ERR              # host: NULL
    assert hk(e.ctx, h0.ctypes.data, h1.ctypes.data, ha.ctypes.data, hk_.ctypes.data, batch, K, 0, 0) == ERR        # host: alpha
    assert hk(e.ctx, h0.ctypes.data, h1.ctypes.data, ha.ctypes.data, hk_.ctypes.data, batch, K, alpha, 0xC00) == ERR  # host: plans
    for flags in (0, 0x400, 0x800, 0x1000):
        assert ks(e.ctx, None, None, None, None, 0, K, alpha, flags, None) == 0            # an empty batch is fine
    assert hk(e.ctx, None, None, None, None, 0, K, alpha, 0) == 0
    # a repeated modulus inside a digit, or among the special rows, is refused by the table builder, on the host
    pr = params(64)
    for idx, kk, al in (([0, 0, 1, 2], 1, 2), ([0, 1, 2, 2], 2, 1)):
        tabs = [np.ascontiguousarray(t[idx]) for t in (pr.P, pr.primitive_roots, pr.invkmax)]
        ctx = C.c_void_p()
        assert Lb.nflhip_ctx_create(C.byref(ctx), 0, 64, N, 4, *[t.ctypes.data_as(C.c_void_p) for t in tabs], pr.kmax_log2) == 0
        try:
            for flags in (0, 0x400, 0x800, 0x1000):
                assert ks(ctx, p0, p1, pa, pk, 1, kk, al, flags, None) == ERR, (idx, flags)
                assert b"baseconv: a source modulus repeats" in Lb.nflhip_last_error(ctx)        # the builder's own message
            assert ks(ctx, None, None, None, None, 0, kk, al, 0, None) == 0                # batch 0 returns before any table is built
        finally:
            torch.cuda.synchronize()
            Lb.nflhip_ctx_destroy(ctx)
    # nothing refused above wrote anything, and the context still works
    torch.cuda.synchronize()
    assert bool((o == 9).all()) and bool((a == 1).all()) and bool((k == 1).all())
    assert ks(e.ctx, p0, p1, pa, pk, batch, K, alpha, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((o != 9).any())


@pytest.fixture(scope="module")
def cpp_program(tmp_path_factory):
    from test_keyswitch_cpu import build_cpp
    return build_cpp(str(tmp_path_factory.mktemp("cpp_keyswitch")), gpu=True)


@pytest.mark.parametrize("batch", [1, 5])
def test_cpp_surface_on_the_gpu(cpp_program, batch):
    """the program of tests/cpp_keyswitch against the real library: poly, poly_p and device_batch equal to the sequence written by hand
    through the existing header calls, and the key used through a device_batch equal to the key used through raw pointers"""
    r = subprocess.run([cpp_program, str(batch)], capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
